// skew_check -- the host twins of the skew estimate and the rotation under AddressSanitizer and UndefinedBehaviorSanitizer, as a
// program of its own (csrc/Makefile: make skew_check).  It runs pseg_skew_maps_host, pseg_rotate_maps_host and pseg_deskew_scans_host
// over seeded maps -- the shapes, steps and densities of tests/test_skew_host.py and shapes drawn at random -- against a per-pixel
// loop: the whole list in one call, then every map alone with its input, its output and its scores placed in exact-size allocations,
// so that a read or write past their ends is caught.  Exit status 0: no mismatch, and the refusals refuse.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../include/pseg.h"
#include "../page-segmentation_amd/csrc/pseg_skew.h"

namespace pseg {                                   // what pseg_skew.hip takes from pseg_engine.hip in the library
std::string& last_error() { static thread_local std::string s; return s; }
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}
}  // namespace pseg

struct Case { int H, W; pseg_skew how; pseg_rotate rot; std::vector<uint8_t> px; };

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                            // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static long long fdiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // floor(a / b), b > 0

// the scores pixel by pixel: every ink pixel (y, x) adds one to P_a[y - off(a, x / 32)]
static int skew_ref(const uint8_t* px, bool from_gray, int H, int W, const pseg_skew& how, std::vector<uint64_t>& scores) {
    const int A = how.steps, D = how.denom, K = (W + 31) / 32;
    long long M = 0;
    for (int a = -A; a <= A; ++a)
        for (int k = 0; k < K; ++k) M = std::max(M, std::llabs(fdiv((long long)a * (64 * k + 32 - W) + D, 2 * D)));
    scores.assign(2 * A + 1, 0);
    int best = 0;
    for (int a = -A; a <= A; ++a) {
        std::vector<long long> P((size_t)(H + 2 * M), 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const uint8_t b = px[(size_t)y * W + x];
                if (from_gray ? b > 127 : b == 0) continue;
                P[(size_t)(y - fdiv((long long)a * (64 * (x / 32) + 32 - W) + D, 2 * D) + M)] += 1;
            }
        uint64_t s = 0;
        for (long long p : P) s += (uint64_t)(p * p);
        scores[a + A] = s;
    }
    for (int a = -A; a <= A; ++a) {
        const uint64_t s = scores[a + A], b = scores[best + A];
        if (s > b || (s == b && (std::abs(a) < std::abs(best) || (std::abs(a) == std::abs(best) && a > best)))) best = a;
    }
    return best;
}

static void rotate_ref(const uint8_t* src, int H, int W, const pseg_rotate& r, std::vector<uint8_t>& out) {
    const double rr = std::sqrt((double)(r.denom * r.denom + r.index * r.index));
    const long long C = (long long)std::floor(16384.0 * r.denom / rr + 0.5);
    long long S = (long long)std::floor(16384.0 * std::abs(r.index) / rr + 0.5);
    if (r.index < 0) S = -S;
    out.assign((size_t)H * W, 0);
    auto tap = [&](long long ys, long long xs) -> long long {
        return ys >= 0 && ys < H && xs >= 0 && xs < W ? src[(size_t)ys * W + xs] : r.fill;
    };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const long long u = 2 * x - (W - 1), v = 2 * y - (H - 1);
            const long long X = C * u - S * v + (long long)(W - 1) * 16384, Y = S * u + C * v + (long long)(H - 1) * 16384;
            long long val;
            if (r.order == 0) val = tap(fdiv(Y + 16384, 32768), fdiv(X + 16384, 32768));
            else {
                const long long x0 = fdiv(X, 32768), y0 = fdiv(Y, 32768), fx = X - x0 * 32768, fy = Y - y0 * 32768, w = 32768;
                val = fdiv((w - fx) * (w - fy) * tap(y0, x0) + fx * (w - fy) * tap(y0, x0 + 1) + (w - fx) * fy * tap(y0 + 1, x0) +
                           fx * fy * tap(y0 + 1, x0 + 1) + (1ll << 29), 1ll << 30);
            }
            out[(size_t)y * W + x] = (uint8_t)val;
        }
}

int main(int argc, char** argv) {
    if (argc > 1) g_state ^= strtoull(argv[1], nullptr, 0);
    const int shapes[][2] = {{1, 1}, {1, 33}, {33, 1}, {2, 31}, {31, 32}, {32, 33}, {64, 65}, {63, 95}, {70, 50}, {129, 257}};
    const int steps[][2] = {{1, 64}, {16, 64}, {89, 1024}, {128, 512}, {128, 4096}};
    const unsigned dens[] = {0, 5, 51, 256};       // ink pixels of 256
    std::vector<Case> cases;
    auto add = [&](int H, int W, int A, int D, unsigned d) {
        const int span = 2 * A + 1;
        Case c{H, W, {A, D}, {(int)(rnd() % span) - A, D, (int)(rnd() & 1), (int)(rnd() % 256)}, std::vector<uint8_t>((size_t)H * W)};
        for (auto& v : c.px) v = (rnd() & 255u) < d ? (uint8_t)(1 + rnd() % 255) : 0;     // non-zero bytes of every value
        cases.push_back(std::move(c));
    };
    for (auto& s : shapes)
        for (auto& t : steps)
            for (unsigned d : dens) add(s[0], s[1], t[0], t[1], d);
    for (int k = 0; k < 60; ++k) {
        const int D = 64 + (int)(rnd() % 4033), A = 1 + (int)(rnd() % std::min(128, D / 4));
        add(1 + (int)(rnd() % 90), 1 + (int)(rnd() % 200), A, D, rnd() % 257);
    }
    const int n = (int)cases.size();
    int bad = 0;
    std::vector<int32_t> index(n, -77), dindex(n, -77);
    std::vector<std::vector<uint64_t>> scores(n);
    std::vector<std::vector<uint8_t>> rot(n), dsk(n);
    {
        std::vector<const uint8_t*> in(n);
        std::vector<int> H(n), W(n);
        std::vector<pseg_skew> how(n);
        std::vector<pseg_rotate> rt(n);
        std::vector<uint64_t*> sp(n);
        std::vector<uint8_t*> rp(n), dp(n);
        for (int i = 0; i < n; ++i) {
            const Case& c = cases[i];
            in[i] = c.px.data(); H[i] = c.H; W[i] = c.W; how[i] = c.how; rt[i] = c.rot;
            scores[i].assign(2 * c.how.steps + 1, 0xA5A5);
            rot[i].assign(c.px.size(), 0xA5);
            dsk[i].assign(c.px.size(), 0xA5);
            sp[i] = scores[i].data(); rp[i] = rot[i].data(); dp[i] = dsk[i].data();
        }
        // refusals first: nothing is written
        const auto keep_rot = rot;
        how[n - 1].steps = 129;
        if (pseg_skew_maps_host(n, in.data(), H.data(), W.data(), how.data(), index.data(), sp.data()) != PSEG_EINVAL || index[0] != -77) { fprintf(stderr, "steps 129 were not refused\n"); ++bad; }
        how[n - 1] = cases[n - 1].how;
        rt[2].order = 2;
        if (pseg_rotate_maps_host(n, in.data(), H.data(), W.data(), rt.data(), rp.data()) != PSEG_EINVAL || rot != keep_rot) { fprintf(stderr, "order 2 was not refused\n"); ++bad; }
        rt[2] = cases[2].rot;
        H[1] = 16385;
        if (pseg_deskew_scans_host(n, in.data(), nullptr, H.data(), W.data(), how.data(), dp.data(), dindex.data()) != PSEG_EINVAL || dindex[0] != -77) { fprintf(stderr, "16385 rows were not refused\n"); ++bad; }
        H[1] = cases[1].H;
        if (pseg_skew_maps_host(n, in.data(), nullptr, W.data(), how.data(), index.data(), sp.data()) != PSEG_EINVAL) { fprintf(stderr, "a NULL array was not refused\n"); ++bad; }
        // the whole lists in one call each
        if (pseg_skew_maps_host(n, in.data(), H.data(), W.data(), how.data(), index.data(), sp.data()) != PSEG_OK ||
            pseg_rotate_maps_host(n, in.data(), H.data(), W.data(), rt.data(), rp.data()) != PSEG_OK ||
            pseg_deskew_scans_host(n, in.data(), nullptr, H.data(), W.data(), how.data(), dp.data(), dindex.data()) != PSEG_OK) {
            fprintf(stderr, "a list call failed: %s\n", pseg::last_error().c_str());
            return 1;
        }
    }
    int turned = 0;
    for (int i = 0; i < n; ++i) {
        const Case& c = cases[i];
        const size_t px = c.px.size();
        std::vector<uint64_t> ws, wg;
        std::vector<uint8_t> wr, wd;
        const int wi = skew_ref(c.px.data(), false, c.H, c.W, c.how, ws);
        const int gi = skew_ref(c.px.data(), true, c.H, c.W, c.how, wg);
        rotate_ref(c.px.data(), c.H, c.W, c.rot, wr);
        rotate_ref(c.px.data(), c.H, c.W, pseg_rotate{gi, c.how.denom, 1, 255}, wd);
        turned += wi != 0;
        if (index[i] != wi || scores[i] != ws) { fprintf(stderr, "case %d (%dx%d, %d/%d): the estimate differs from the per-pixel loop\n", i, c.H, c.W, c.how.steps, c.how.denom); ++bad; }
        if (rot[i] != wr) { fprintf(stderr, "case %d (%dx%d, index %d/%d order %d): the rotation differs from the per-pixel loop\n", i, c.H, c.W, c.rot.index, c.rot.denom, c.rot.order); ++bad; }
        if (dindex[i] != gi || dsk[i] != wd) { fprintf(stderr, "case %d: the combined entry differs from the per-pixel loop\n", i); ++bad; }
        // alone, from and into exact-size allocations; the combined entry with the map as its own ink map
        uint8_t* in = (uint8_t*)malloc(px);
        uint8_t* op = (uint8_t*)malloc(px);
        uint64_t* sc = (uint64_t*)malloc(ws.size() * sizeof(uint64_t));
        memcpy(in, c.px.data(), px);
        const uint8_t* ip = in;
        int32_t one = -77;
        if (pseg_skew_maps_host(1, &ip, &c.H, &c.W, &c.how, &one, &sc) != PSEG_OK || one != wi || memcmp(sc, ws.data(), ws.size() * sizeof(uint64_t)) != 0) { fprintf(stderr, "case %d: the estimate alone differs\n", i); ++bad; }
        if (pseg_skew_maps_host(1, &ip, &c.H, &c.W, &c.how, &one, nullptr) != PSEG_OK || one != wi) { fprintf(stderr, "case %d: the estimate without scores differs\n", i); ++bad; }
        if (pseg_rotate_maps_host(1, &ip, &c.H, &c.W, &c.rot, &op) != PSEG_OK || memcmp(op, wr.data(), px) != 0) { fprintf(stderr, "case %d: the rotation alone differs\n", i); ++bad; }
        rotate_ref(c.px.data(), c.H, c.W, pseg_rotate{wi, c.how.denom, 1, 255}, wd);
        if (pseg_deskew_scans_host(1, &ip, &ip, &c.H, &c.W, &c.how, &op, &one) != PSEG_OK || one != wi || memcmp(op, wd.data(), px) != 0) { fprintf(stderr, "case %d: the combined entry with an ink map differs\n", i); ++bad; }
        const pseg_rotate ident = {0, c.how.denom, (int)(i & 1), 9};
        if (pseg_rotate_maps_host(1, &ip, &c.H, &c.W, &ident, &op) != PSEG_OK || memcmp(op, in, px) != 0) { fprintf(stderr, "case %d: index 0 is not the identity\n", i); ++bad; }
        free(sc);
        free(op);
        free(in);
    }
    printf("skew_check: %d cases against a per-pixel loop (%d with a skew), %d mismatches\n", n, turned, bad);
    return bad ? 1 : 0;
}
