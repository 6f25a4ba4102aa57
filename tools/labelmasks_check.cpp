// labelmasks_check -- the label-map loader's host entry under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its
// own (csrc/Makefile: make labelmasks_check).  It runs pseg_label_masks_host over a few hundred seeded cases -- source and output
// shapes, both channel counts, tables of 0 .. 256 colours -- as one list, then every mask alone with its source and its outputs in
// exact-size allocations, so that a read or write past the arrays is caught, and compares labels and counts with a plain loop that
// looks the colour up first and gathers second.  Exit status 0: no mismatch, and the refusals refuse.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pseg.h"
#include "../page-segmentation_amd/csrc/pseg_labelmasks.h"

namespace pseg {                                   // what pseg_labelmasks.hip takes from pseg_engine.hip in the library
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

struct Case { int H0, W0, ch, H, W, n_colors; std::vector<uint8_t> px; };

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                            // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// the whole mask to ids first (every table entry compared, the last match wins: there are no duplicates), then the gather
static void plain(const Case& c, const uint8_t* colors, const uint8_t* ids, std::vector<uint8_t>& lab, std::vector<int64_t>& cnt) {
    const size_t n0 = (size_t)c.H0 * c.W0;
    std::vector<uint8_t> id0(n0), unk0(n0, 0);
    for (size_t p = 0; p < n0; ++p) {
        if (c.ch == 1) { id0[p] = c.px[p]; continue; }
        id0[p] = 0; unk0[p] = 1;
        for (int k = 0; k < c.n_colors; ++k)
            if (memcmp(&c.px[3 * p], &colors[3 * k], 3) == 0) { id0[p] = ids[k]; unk0[p] = 0; }
    }
    double fy, ty, fx, tx;
    pseg::lm_coeffs(c.H0, c.H, &fy, &ty);
    pseg::lm_coeffs(c.W0, c.W, &fx, &tx);
    lab.assign((size_t)c.H * c.W, 0);
    cnt.assign(257, 0);
    for (int r = 0; r < c.H; ++r)
        for (int x = 0; x < c.W; ++x) {
            const size_t p = (size_t)pseg::lm_src_index(r, fy, ty, c.H0) * c.W0 + pseg::lm_src_index(x, fx, tx, c.W0);
            lab[(size_t)r * c.W + x] = id0[p];
            ++cnt[id0[p]];
            cnt[256] += unk0[p];
        }
}

int main(int argc, char** argv) {
    if (argc > 1) g_state ^= strtoull(argv[1], nullptr, 0);
    // 256 distinct colours, neighbours that differ by 1 in one channel among them; ids in no order, 0 among them
    std::vector<uint8_t> colors(256 * 3), ids(256);
    for (int k = 0; k < 256; ++k) {
        colors[3 * k] = (uint8_t)(k & 3); colors[3 * k + 1] = (uint8_t)((k >> 2) & 7); colors[3 * k + 2] = (uint8_t)(k >> 5);
        ids[k] = (uint8_t)((k * 37 + 11) & 255);
    }
    const int shapes[][4] = {{1, 1, 1, 1}, {1, 37, 1, 19}, {33, 1, 70, 1}, {70, 50, 35, 25}, {35, 25, 70, 50}, {64, 48, 64, 48}, {97, 131, 41, 77},
                             {5, 9, 3, 7}, {5, 9, 11, 8}, {5, 9, 2, 9}, {40, 30, 13, 255}, {40, 30, 9, 256}, {40, 30, 9, 257}, {12, 300, 17, 263}};
    const int tables[] = {0, 1, 3, 8, 17, 256};
    std::vector<Case> cases;
    for (int rep = 0; rep < 3; ++rep)
        for (auto& s : shapes)
            for (int nc : tables)
                for (int ch : {3, 1}) {
                    if (ch == 1 && nc != 3 && nc != 256) continue;
                    Case c{s[0], s[1], ch, s[2], s[3], nc, std::vector<uint8_t>((size_t)s[0] * s[1] * ch)};
                    if (ch == 1) for (auto& v : c.px) v = (uint8_t)rnd();
                    else
                        for (size_t p = 0; p < c.px.size(); p += 3) {                  // mostly table colours, some unknown ones
                            const unsigned k = rnd() % (unsigned)(nc + 2);
                            if ((int)k < nc) memcpy(&c.px[p], &colors[3 * k], 3);
                            else { c.px[p] = (uint8_t)(200 + rnd() % 50); c.px[p + 1] = (uint8_t)rnd(); c.px[p + 2] = (uint8_t)rnd(); }
                        }
                    cases.push_back(std::move(c));
                }
    const int n = (int)cases.size();
    int bad = 0;
    long long pixels = 0;
    // lists: the cases of one table size in one call (the table belongs to the call)
    std::vector<std::vector<uint8_t>> lab(n);
    std::vector<std::vector<int64_t>> cnt(n);
    for (int nc : tables) {
        std::vector<int> which;
        for (int i = 0; i < n; ++i) if (cases[i].n_colors == nc) which.push_back(i);
        const int m = (int)which.size();
        std::vector<pseg_mask_src> src(m);
        std::vector<int> H(m), W(m);
        std::vector<uint8_t*> out(m);
        std::vector<int64_t> counts((size_t)m * 257, -1);
        for (int k = 0; k < m; ++k) {
            const Case& c = cases[which[k]];
            lab[which[k]].assign((size_t)c.H * c.W, 0xA5);
            src[k] = {c.px.data(), c.H0, c.W0, c.ch};
            H[k] = c.H; W[k] = c.W; out[k] = lab[which[k]].data();
        }
        if (pseg_label_masks_host(m, src.data(), H.data(), W.data(), colors.data(), ids.data(), nc, out.data(), counts.data()) != PSEG_OK) {
            fprintf(stderr, "the list call with %d colours failed: %s\n", nc, pseg::last_error().c_str());
            return 1;
        }
        for (int k = 0; k < m; ++k) cnt[which[k]].assign(counts.begin() + (size_t)k * 257, counts.begin() + (size_t)(k + 1) * 257);
        // refusals: nothing is written
        const std::vector<uint8_t> keep = lab[which[0]];
        const std::vector<int64_t> keepc = counts;
        auto refused = [&](const char* what, int rc) {
            if (rc != PSEG_EINVAL || lab[which[0]] != keep || counts != keepc) { fprintf(stderr, "%s was not refused cleanly\n", what); ++bad; }
        };
        src[m - 1].channels = 4;
        refused("4 channels", pseg_label_masks_host(m, src.data(), H.data(), W.data(), colors.data(), ids.data(), nc, out.data(), counts.data()));
        src[m - 1].channels = cases[which[m - 1]].ch;
        W[m - 1] = 0;
        refused("an empty output shape", pseg_label_masks_host(m, src.data(), H.data(), W.data(), colors.data(), ids.data(), nc, out.data(), counts.data()));
        W[m - 1] = cases[which[m - 1]].W;
        refused("257 colours", pseg_label_masks_host(m, src.data(), H.data(), W.data(), colors.data(), ids.data(), 257, out.data(), counts.data()));
        refused("a NULL array", pseg_label_masks_host(m, src.data(), nullptr, W.data(), colors.data(), ids.data(), nc, out.data(), counts.data()));
        if (nc >= 3) {
            std::vector<uint8_t> dup(colors.begin(), colors.begin() + 3 * nc);
            memcpy(&dup[3 * (nc - 1)], &dup[3], 3);
            refused("a duplicate colour", pseg_label_masks_host(m, src.data(), H.data(), W.data(), dup.data(), ids.data(), nc, out.data(), counts.data()));
        }
    }
    for (int i = 0; i < n; ++i) {
        const Case& c = cases[i];
        const size_t npx = (size_t)c.H * c.W;
        // alone, from and into exact-size allocations; the counts off for every third case
        uint8_t* px = (uint8_t*)malloc(c.px.size());
        uint8_t* out = (uint8_t*)malloc(npx);
        int64_t* counts = (int64_t*)malloc(257 * sizeof(int64_t));
        uint8_t* col = (uint8_t*)malloc(c.n_colors ? 3 * (size_t)c.n_colors : 1);
        uint8_t* idv = (uint8_t*)malloc(c.n_colors ? (size_t)c.n_colors : 1);
        memcpy(px, c.px.data(), c.px.size());
        memcpy(col, colors.data(), 3 * (size_t)c.n_colors);
        memcpy(idv, ids.data(), (size_t)c.n_colors);
        const pseg_mask_src src = {px, c.H0, c.W0, c.ch};
        const bool with = i % 3 != 2;
        if (pseg_label_masks_host(1, &src, &c.H, &c.W, c.n_colors ? col : nullptr, c.n_colors ? idv : nullptr, c.n_colors, &out, with ? counts : nullptr) != PSEG_OK) {
            fprintf(stderr, "case %d: the call failed: %s\n", i, pseg::last_error().c_str());
            ++bad;
        } else {
            std::vector<uint8_t> want;
            std::vector<int64_t> wantc;
            plain(c, colors.data(), ids.data(), want, wantc);
            if (memcmp(out, want.data(), npx) != 0) { fprintf(stderr, "case %d (%dx%dx%d -> %dx%d, %d colours): labels differ from the plain loop\n", i, c.H0, c.W0, c.ch, c.H, c.W, c.n_colors); ++bad; }
            if (memcmp(out, lab[i].data(), npx) != 0) { fprintf(stderr, "case %d: alone and in the list differ\n", i); ++bad; }
            if (with && memcmp(counts, wantc.data(), 257 * sizeof(int64_t)) != 0) { fprintf(stderr, "case %d: counts differ from the plain loop\n", i); ++bad; }
            if (cnt[i] != wantc) { fprintf(stderr, "case %d: the list's counts differ from the plain loop\n", i); ++bad; }
            pixels += (long long)npx;
        }
        free(idv); free(col); free(counts); free(out); free(px);
    }
    printf("labelmasks_check: %d cases, %lld pixels compared with the plain loop, %d mismatches\n", n, pixels, bad);
    return bad ? 1 : 0;
}
