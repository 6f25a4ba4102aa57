// despeckle_check -- the despeckling's host entry under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
// (csrc/Makefile: make despeckle_check).  It runs pseg_despeckle_maps_host over seeded maps -- the shape x connectivity x max_area x
// density grid of tests/test_despeckle_host.py and shapes drawn at random -- against a plain flood fill: the whole list in one call,
// then every map alone with its input and its output placed in exact-size allocations, so that a read or write past H * W bytes is
// caught, and once more in place.  Exit status 0: no mismatch, and the refusals refuse.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pseg.h"
#include "../page-segmentation_amd/csrc/pseg_despeckle.h"

namespace pseg {                                   // what pseg_despeckle.hip takes from pseg_engine.hip in the library
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

struct Case { int H, W; pseg_despeckle how; std::vector<uint8_t> px; };

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                            // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// the components by a flood fill with an explicit stack: out and counts as the contract states them
static void flood(const Case& c, std::vector<uint8_t>& out, int64_t counts[3]) {
    const int H = c.H, W = c.W;
    std::vector<int> lab((size_t)H * W, -1), stack;
    std::vector<unsigned> size;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            if (!c.px[o] || lab[o] >= 0) continue;
            const int id = (int)size.size();
            size.push_back(0);
            lab[o] = id;
            stack.push_back((int)o);
            while (!stack.empty()) {
                const int q = stack.back();
                stack.pop_back();
                ++size[id];
                const int qy = q / W, qx = q % W;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((dy == 0 && dx == 0) || (c.how.connectivity == 4 && dy != 0 && dx != 0)) continue;
                        const int ny = qy + dy, nx = qx + dx;
                        if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                        const size_t p = (size_t)ny * W + nx;
                        if (c.px[p] && lab[p] < 0) { lab[p] = id; stack.push_back((int)p); }
                    }
            }
        }
    counts[0] = counts[1] = counts[2] = 0;
    for (unsigned s : size) {
        if (pseg::ds_speck(s, c.how.max_area)) { ++counts[0]; counts[1] += s; } else ++counts[2];
    }
    out.assign((size_t)H * W, 0);
    for (size_t o = 0; o < out.size(); ++o) out[o] = lab[o] >= 0 && !pseg::ds_speck(size[lab[o]], c.how.max_area);
}

int main(int argc, char** argv) {
    if (argc > 1) g_state ^= strtoull(argv[1], nullptr, 0);
    const int shapes[][2] = {{1, 1}, {1, 37}, {33, 1}, {2, 2}, {31, 65}, {32, 64}, {33, 63}, {64, 128}, {70, 50}, {97, 130}};
    const int areas[] = {1, 2, 9, 64, 5000};
    const unsigned dens[] = {13, 77, 180, 230};    // ink pixels of 256
    std::vector<Case> cases;
    auto add = [&](int H, int W, int area, int conn, unsigned d) {
        Case c{H, W, {area, conn}, std::vector<uint8_t>((size_t)H * W)};
        for (auto& v : c.px) v = (rnd() & 255u) < d ? (uint8_t)(1 + rnd() % 255) : 0;     // non-zero bytes of every value
        cases.push_back(std::move(c));
    };
    for (auto& s : shapes)
        for (int conn : {4, 8})
            for (int a : areas)
                for (unsigned d : dens) add(s[0], s[1], a, conn, d);
    for (int k = 0; k < 120; ++k) add(1 + (int)(rnd() % 90), 1 + (int)(rnd() % 150), 1 + (int)(rnd() % 40), (rnd() & 1) ? 4 : 8, 20 + rnd() % 200);
    const int n = (int)cases.size();
    int bad = 0;
    // the whole list in one call
    std::vector<std::vector<uint8_t>> out(n);
    std::vector<int64_t> counts((size_t)n * 3, -7);
    {
        std::vector<const uint8_t*> in(n);
        std::vector<int> H(n), W(n);
        std::vector<pseg_despeckle> how(n);
        std::vector<uint8_t*> op(n);
        for (int i = 0; i < n; ++i) {
            out[i].assign(cases[i].px.size(), 0xA5);
            in[i] = cases[i].px.data(); H[i] = cases[i].H; W[i] = cases[i].W; how[i] = cases[i].how;
            op[i] = out[i].data();
        }
        if (pseg_despeckle_maps_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), counts.data()) != PSEG_OK) {
            fprintf(stderr, "the list call failed: %s\n", pseg::last_error().c_str());
            return 1;
        }
        // refusals: nothing is written
        std::vector<std::vector<uint8_t>> keep = out;
        const std::vector<int64_t> keep_counts = counts;
        how[n - 1].connectivity = 3;
        if (pseg_despeckle_maps_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), counts.data()) != PSEG_EINVAL || out != keep || counts != keep_counts) { fprintf(stderr, "connectivity 3 was not refused\n"); ++bad; }
        how[n - 1] = cases[n - 1].how;
        how[2].max_area = pseg::DS_AREA_MAX + 1;
        if (pseg_despeckle_maps_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), counts.data()) != PSEG_EINVAL || out != keep) { fprintf(stderr, "a max_area above the range was not refused\n"); ++bad; }
        how[2] = cases[2].how;
        H[1] = 0;
        if (pseg_despeckle_maps_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), counts.data()) != PSEG_EINVAL || out != keep) { fprintf(stderr, "an empty shape was not refused\n"); ++bad; }
        if (pseg_despeckle_maps_host(n, in.data(), nullptr, W.data(), how.data(), op.data(), counts.data()) != PSEG_EINVAL) { fprintf(stderr, "a NULL array was not refused\n"); ++bad; }
    }
    long long erased = 0, kept = 0;
    for (int i = 0; i < n; ++i) {
        const Case& c = cases[i];
        const size_t px = c.px.size();
        std::vector<uint8_t> want;
        int64_t wc[3];
        flood(c, want, wc);
        erased += wc[0];
        kept += wc[2];
        if (out[i] != want || memcmp(wc, &counts[(size_t)i * 3], sizeof wc) != 0) {
            fprintf(stderr, "case %d (%dx%d, max_area %d, connectivity %d): the list call differs from the flood fill\n", i, c.H, c.W, c.how.max_area, c.how.connectivity);
            ++bad;
        }
        // alone, from and into exact-size allocations; then in place; then not despeckled
        uint8_t* in = (uint8_t*)malloc(px);
        uint8_t* op = (uint8_t*)malloc(px);
        memcpy(in, c.px.data(), px);
        const uint8_t* ip = in;
        int64_t one[3] = {-7, -7, -7};
        if (pseg_despeckle_maps_host(1, &ip, &c.H, &c.W, &c.how, &op, one) != PSEG_OK) { fprintf(stderr, "case %d: the call failed\n", i); ++bad; }
        else if (memcmp(op, want.data(), px) != 0 || memcmp(one, wc, sizeof wc) != 0) { fprintf(stderr, "case %d: alone and in the list differ\n", i); ++bad; }
        if (pseg_despeckle_maps_host(1, &ip, &c.H, &c.W, &c.how, &in, nullptr) != PSEG_OK || memcmp(in, want.data(), px) != 0) { fprintf(stderr, "case %d: in place differs\n", i); ++bad; }
        memcpy(in, c.px.data(), px);
        const pseg_despeckle none = {0, 0};
        if (pseg_despeckle_maps_host(1, &ip, &c.H, &c.W, &none, &op, one) != PSEG_OK || memcmp(op, c.px.data(), px) != 0 || one[0] || one[1] || one[2]) { fprintf(stderr, "case %d: max_area 0 changed the map\n", i); ++bad; }
        free(op);
        free(in);
    }
    printf("despeckle_check: %d cases against a flood fill (%lld components erased, %lld kept), %d mismatches\n", n, erased, kept, bad);
    return bad ? 1 : 0;
}
