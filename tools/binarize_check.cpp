// binarize_check -- the binarisation's host entry under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
// (csrc/Makefile: make binarize_check).  It runs pseg_binarize_scans_host over the shape x window x k grid of
// tests/test_binarize_host.py with pixels from a seed: the whole list in one call, then every scan alone with its input and its
// outputs placed in exact-size allocations, so that a read or write past H * W elements is caught.  Where the window is small
// enough the result is compared with sums taken pixel by pixel over the mirrored window (the decision function is the header's).
// Exit status 0: no mismatch, and the refusals refuse.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pseg.h"
#include "../page-segmentation_amd/csrc/pseg_binarize.h"

namespace pseg {                                   // what pseg_binarize.hip takes from pseg_engine.hip in the library
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

struct Case { int H, W; pseg_binarize how; std::vector<uint8_t> px; };

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                            // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// the window's sums pixel by pixel
static bool direct(const Case& c, int y, int x, double* T) {
    const int r = c.how.window / 2;
    unsigned long long packed = 0;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx)
            packed += pseg::bz_pack(c.px[(size_t)pseg::bz_mirror(y + dy, c.H) * c.W + pseg::bz_mirror(x + dx, c.W)]);
    return pseg::bz_decide(packed, c.px[(size_t)y * c.W + x], (double)c.how.window * c.how.window, c.how.k, c.how.R, T);
}

int main(int argc, char** argv) {
    if (argc > 1) g_state ^= strtoull(argv[1], nullptr, 0);
    const int shapes[][2] = {{1, 1}, {1, 37}, {33, 1}, {2, 2}, {5, 7}, {31, 65}, {64, 128}, {70, 50}, {97, 130}};
    const int windows[] = {3, 15, 37, 255, 0};
    const double ks[] = {0.0, 0.2, 0.5};
    const unsigned dens[] = {13, 77, 180};         // dark pixels of 256
    std::vector<Case> cases;
    for (auto& s : shapes)
        for (int w : windows)
            for (double k : ks)
                for (unsigned d : dens) {
                    Case c{s[0], s[1], {w, k, 128.0}, std::vector<uint8_t>((size_t)s[0] * s[1])};
                    for (auto& v : c.px) v = (uint8_t)((rnd() & 255u) < d ? rnd() % 120 : 130 + rnd() % 126);
                    cases.push_back(std::move(c));
                }
    const int n = (int)cases.size();
    int bad = 0;
    // the whole list in one call
    std::vector<std::vector<uint8_t>> ink(n);
    std::vector<std::vector<double>> thr(n);
    {
        std::vector<const uint8_t*> g(n);
        std::vector<int> H(n), W(n);
        std::vector<pseg_binarize> how(n);
        std::vector<uint8_t*> oi(n);
        std::vector<double*> ot(n);
        for (int i = 0; i < n; ++i) {
            ink[i].assign(cases[i].px.size(), 0xA5);
            thr[i].assign(cases[i].px.size(), -7.0);
            g[i] = cases[i].px.data(); H[i] = cases[i].H; W[i] = cases[i].W; how[i] = cases[i].how;
            oi[i] = ink[i].data();
            ot[i] = i % 4 == 3 ? nullptr : thr[i].data();      // an entry of the threshold array may be NULL
        }
        if (pseg_binarize_scans_host(n, g.data(), H.data(), W.data(), how.data(), oi.data(), ot.data()) != PSEG_OK) {
            fprintf(stderr, "the list call failed: %s\n", pseg::last_error().c_str());
            return 1;
        }
        // refusals: nothing is written
        std::vector<uint8_t> keep = ink[0];
        how[n - 1].window = 14;
        if (pseg_binarize_scans_host(n, g.data(), H.data(), W.data(), how.data(), oi.data(), ot.data()) != PSEG_EINVAL || ink[0] != keep) { fprintf(stderr, "an even window was not refused\n"); ++bad; }
        how[n - 1] = cases[n - 1].how;
        H[1] = 0;
        if (pseg_binarize_scans_host(n, g.data(), H.data(), W.data(), how.data(), oi.data(), ot.data()) != PSEG_EINVAL) { fprintf(stderr, "an empty shape was not refused\n"); ++bad; }
        if (pseg_binarize_scans_host(n, g.data(), nullptr, W.data(), how.data(), oi.data(), ot.data()) != PSEG_EINVAL) { fprintf(stderr, "a NULL array was not refused\n"); ++bad; }
    }
    long long compared = 0;
    for (int i = 0; i < n; ++i) {
        const Case& c = cases[i];
        const size_t px = c.px.size();
        // alone, from and into exact-size allocations
        uint8_t* g = (uint8_t*)malloc(px);
        uint8_t* oi = (uint8_t*)malloc(px);
        double* ot = (double*)malloc(px * sizeof(double));
        memcpy(g, c.px.data(), px);
        const uint8_t* gp = g;
        if (pseg_binarize_scans_host(1, &gp, &c.H, &c.W, &c.how, &oi, &ot) != PSEG_OK) { fprintf(stderr, "case %d: the call failed\n", i); ++bad; }
        else {
            if (memcmp(oi, ink[i].data(), px) != 0) { fprintf(stderr, "case %d: alone and in the list differ\n", i); ++bad; }
            if (i % 4 != 3 && memcmp(ot, thr[i].data(), px * sizeof(double)) != 0) { fprintf(stderr, "case %d: thresholds alone and in the list differ\n", i); ++bad; }
            if (i % 4 == 3 && thr[i][0] != -7.0) { fprintf(stderr, "case %d: a NULL threshold entry was written\n", i); ++bad; }
            if (c.how.window == 0) {
                for (size_t o = 0; o < px; ++o)
                    if (oi[o] != (c.px[o] <= 127) || ot[o] != 127.0) { fprintf(stderr, "case %d: fixed threshold differs\n", i); ++bad; break; }
            } else if ((long long)px * c.how.window * c.how.window <= 40000000LL) {
                for (int y = 0; y < c.H && !bad; ++y)
                    for (int x = 0; x < c.W; ++x) {
                        double T;
                        const bool want = direct(c, y, x, &T);
                        if (oi[(size_t)y * c.W + x] != (uint8_t)want || memcmp(&T, &ot[(size_t)y * c.W + x], 8) != 0) {
                            fprintf(stderr, "case %d (%dx%d, window %d): pixel (%d,%d) differs\n", i, c.H, c.W, c.how.window, y, x);
                            ++bad;
                            break;
                        }
                    }
                ++compared;
            }
        }
        free(ot);
        free(oi);
        free(g);
    }
    printf("binarize_check: %d cases, %lld compared pixel by pixel, %d mismatches\n", n, compared, bad);
    return bad ? 1 : 0;
}
