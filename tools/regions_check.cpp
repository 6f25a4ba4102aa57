// regions_check -- the text regions' host entry and the polygon tracer under AddressSanitizer and UndefinedBehaviorSanitizer, as a
// program of its own (csrc/Makefile: make regions_check).  It runs pseg_text_regions_host over seeded label maps -- the shapes and side
// triples of tests/test_regions_host.py and shapes drawn at random -- against a plain per-pixel loop (every window offset spelled out,
// no words, no separable passes) and a flood fill: the whole list in one call, then every map alone with its input, its mask and its
// table placed in exact-size allocations, so that a read or write past them is caught; then pseg_trace_regions_host with exact-size
// vertex and offset arrays, the shoelace area of every polygon of a region without an island against the table, and the cap protocol;
// then pseg_text_regions_poly_host -- the word-run walk over bit planes that the device tracer shares (pseg_regions.h) -- against those
// polygons, again from exact-size arrays and with its capacity protocol.
// Exit status 0: no mismatch, and the refusals refuse.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pseg.h"
#include "../page-segmentation_amd/csrc/pseg_regions.h"

namespace pseg {                                   // what pseg_regions.hip takes from pseg_engine.hip in the library
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

struct Case { int H, W; pseg_regions how; std::vector<uint8_t> px; };

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                            // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

typedef std::vector<uint8_t> Map;

// one rectangle operation, pixel by pixel: OR (dilation, 0 outside) or AND (erosion, 1 outside) over the k x k offsets d - k/2
static Map rect(const Map& m, int H, int W, int k, bool ero) {
    Map out((size_t)H * W);
    const int a = k / 2;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool v = ero;
            for (int dy = 0; dy < k && v == ero; ++dy)
                for (int dx = 0; dx < k; ++dx) {
                    const int yy = y + dy - a, xx = x + dx - a;
                    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                    const bool s = in ? m[(size_t)yy * W + xx] != 0 : ero;
                    if (s != ero) { v = !ero; break; }
                }
            out[(size_t)y * W + x] = v;
        }
    return out;
}

// 4-connected components of the set pixels by a flood fill: ids in raster order of their first pixel
static int flood(const Map& m, int H, int W, std::vector<int>& lab) {
    lab.assign((size_t)H * W, -1);
    std::vector<int> stack;
    int n = 0;
    for (int o = 0; o < H * W; ++o) {
        if (!m[o] || lab[o] >= 0) continue;
        lab[o] = n;
        stack.push_back(o);
        while (!stack.empty()) {
            const int q = stack.back();
            stack.pop_back();
            const int qy = q / W, qx = q % W;
            const int ny[4] = {qy - 1, qy + 1, qy, qy}, nx[4] = {qx, qx, qx - 1, qx + 1};
            for (int d = 0; d < 4; ++d) {
                if (ny[d] < 0 || ny[d] >= H || nx[d] < 0 || nx[d] >= W) continue;
                const int p = ny[d] * W + nx[d];
                if (m[p] && lab[p] < 0) { lab[p] = n; stack.push_back(p); }
            }
        }
        ++n;
    }
    return n;
}

static void expected(const Case& c, Map& T, std::vector<int32_t>& rows) {
    const int H = c.H, W = c.W;
    Map m((size_t)H * W);
    for (size_t o = 0; o < m.size(); ++o) m[o] = c.px[o] == c.how.label;
    m = rect(rect(m, H, W, c.how.k_close, false), H, W, c.how.k_close, true);
    const Map m3 = rect(rect(m, H, W, c.how.k_open, true), H, W, c.how.k_open, false);
    const Map rt = rect(rect(rect(m3, H, W, c.how.k_join, false), H, W, c.how.k_join, false), H, W, c.how.k_join, true);
    Map bg((size_t)H * W);
    for (size_t o = 0; o < bg.size(); ++o) bg[o] = !rt[o];
    std::vector<int> lab;
    const int nb = flood(bg, H, W, lab);
    std::vector<uint8_t> edge(nb, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (lab[(size_t)y * W + x] >= 0 && (y == 0 || y == H - 1 || x == 0 || x == W - 1)) edge[lab[(size_t)y * W + x]] = 1;
    T.assign((size_t)H * W, 0);
    for (size_t o = 0; o < T.size(); ++o) T[o] = m3[o] || rt[o] || (lab[o] >= 0 && !edge[lab[o]]);
    const int n = flood(T, H, W, lab);
    rows.assign((size_t)n * 8, 0);
    std::vector<uint8_t> seen(n, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int l = lab[(size_t)y * W + x];
            if (l < 0) continue;
            int32_t* const r = rows.data() + (size_t)l * 8;
            if (!seen[l]) { seen[l] = 1; r[0] = x; r[1] = y; r[2] = x + 1; r[3] = y + 1; r[5] = y; r[6] = x; }
            if (x < r[0]) r[0] = x;
            if (x + 1 > r[2]) r[2] = x + 1;
            if (y + 1 > r[3]) r[3] = y + 1;
            ++r[4];
        }
}

// does the region of this seed enclose background (an island)?  The outside is what a flood of everything but the region reaches
// from the map's edge, 8-connected (the walk keeps diagonal pixels apart)
static bool has_island(const Map& T, int H, int W, const std::vector<int>& lab, int l) {
    std::vector<uint8_t> out((size_t)H * W, 0);
    std::vector<int> stack;
    auto push = [&](int y, int x) {
        if (y < 0 || y >= H || x < 0 || x >= W) return;
        const int o = y * W + x;
        if (lab[o] == l || out[o]) return;
        out[o] = 1;
        stack.push_back(o);
    };
    for (int y = 0; y < H; ++y) { push(y, 0); push(y, W - 1); }
    for (int x = 0; x < W; ++x) { push(0, x); push(H - 1, x); }
    while (!stack.empty()) {
        const int q = stack.back();
        stack.pop_back();
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) push(q / W + dy, q % W + dx);
    }
    for (size_t o = 0; o < out.size(); ++o)
        if (lab[o] != l && !out[o]) return true;
    return false;
}

int main(int argc, char** argv) {
    if (argc > 1) g_state ^= strtoull(argv[1], nullptr, 0);
    const int shapes[][2] = {{1, 1}, {1, 70}, {70, 1}, {31, 63}, {32, 64}, {33, 65}, {63, 127}, {64, 128}, {65, 129}, {50, 200}};
    const int triples[][3] = {{1, 1, 1}, {2, 2, 2}, {3, 1, 2}, {4, 1, 3}, {7, 2, 6}, {11, 3, 10}, {12, 4, 10}, {23, 7, 20}, {40, 13, 36},
                              {64, 21, 58}, {65, 22, 59}, {255, 85, 231}};
    const unsigned dens[] = {40, 110, 180};        // label pixels of 256, in blocks
    std::vector<Case> cases;
    auto add = [&](int H, int W, const int* k, unsigned d, int block) {
        Case c{H, W, {(int)(rnd() % 3), k[0], k[1], k[2]}, std::vector<uint8_t>((size_t)H * W)};
        const int bw = (W + block - 1) / block;
        std::vector<uint8_t> on((size_t)((H + block - 1) / block) * bw);
        for (auto& v : on) v = (rnd() & 255u) < d;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const bool s = on[(size_t)(y / block) * bw + x / block] != ((rnd() & 31u) == 0);
                c.px[(size_t)y * W + x] = (uint8_t)(s ? c.how.label : (c.how.label + 1 + rnd() % 2) % 3 + (rnd() % 8 == 0 ? 200 : 0));
            }
        cases.push_back(std::move(c));
    };
    for (auto& s : shapes)
        for (auto& k : triples)
            for (unsigned d : dens) {
                if ((long long)s[0] * s[1] * k[0] * k[0] > 300000000LL) continue;      // the per-pixel loop is k^2 per pixel
                add(s[0], s[1], k, d, 1 + k[0] / 3);
            }
    for (int i = 0; i < 80; ++i) {
        const int k[3] = {1 + (int)(rnd() % 14), 1 + (int)(rnd() % 6), 1 + (int)(rnd() % 12)};
        add(1 + (int)(rnd() % 90), 1 + (int)(rnd() % 150), k, 30 + rnd() % 180, 1 + (int)(rnd() % 6));
    }
    const int n = (int)cases.size();
    int bad = 0;
    const int cap = 4096;
    // the whole list in one call
    std::vector<Map> out(n);
    std::vector<int32_t> table((size_t)n * cap * 8, -7);
    std::vector<int> count(n, -7);
    {
        std::vector<const uint8_t*> in(n);
        std::vector<int> H(n), W(n);
        std::vector<pseg_regions> how(n);
        std::vector<uint8_t*> op(n);
        for (int i = 0; i < n; ++i) {
            out[i].assign(cases[i].px.size(), 0xA5);
            in[i] = cases[i].px.data(); H[i] = cases[i].H; W[i] = cases[i].W; how[i] = cases[i].how;
            op[i] = out[i].data();
        }
        if (pseg_text_regions_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), cap, table.data(), count.data()) != PSEG_OK) {
            fprintf(stderr, "the list call failed: %s\n", pseg::last_error().c_str());
            return 1;
        }
        // refusals: nothing is written
        const std::vector<Map> keep = out;
        const std::vector<int32_t> keep_table = table;
        const std::vector<int> keep_count = count;
        auto same = [&]() { return out == keep && table == keep_table && count == keep_count; };
        how[n - 1].k_open = 0;
        if (pseg_text_regions_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), cap, table.data(), count.data()) != PSEG_EINVAL || !same()) { fprintf(stderr, "a side of 0 was not refused\n"); ++bad; }
        how[n - 1] = cases[n - 1].how;
        how[2].k_join = 256;
        if (pseg_text_regions_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), cap, table.data(), count.data()) != PSEG_EINVAL || !same()) { fprintf(stderr, "a side of 256 was not refused\n"); ++bad; }
        how[2] = cases[2].how;
        H[1] = 0;
        if (pseg_text_regions_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), cap, table.data(), count.data()) != PSEG_EINVAL || !same()) { fprintf(stderr, "an empty shape was not refused\n"); ++bad; }
        H[1] = 1 << 16; W[1] = 1 << 15;
        if (pseg_text_regions_host(n, in.data(), H.data(), W.data(), how.data(), op.data(), cap, table.data(), count.data()) != PSEG_EUNSUPPORTED || !same()) { fprintf(stderr, "2^31 pixels were not refused\n"); ++bad; }
        if (pseg_text_regions_host(n, in.data(), nullptr, W.data(), how.data(), op.data(), cap, table.data(), count.data()) != PSEG_EINVAL) { fprintf(stderr, "a NULL array was not refused\n"); ++bad; }
    }
    long long regions = 0, vertices = 0, islands = 0, twins = 0;
    for (int i = 0; i < n; ++i) {
        const Case& c = cases[i];
        const size_t px = c.px.size();
        Map want;
        std::vector<int32_t> rows;
        expected(c, want, rows);
        const int r = (int)(rows.size() / 8);
        regions += r;
        if (out[i] != want || count[i] != r || (r > 0 && r <= cap && memcmp(rows.data(), &table[(size_t)i * cap * 8], rows.size() * 4) != 0)) {
            fprintf(stderr, "case %d (%dx%d, sides %d %d %d): the list call differs from the per-pixel loop\n", i, c.H, c.W, c.how.k_close, c.how.k_open, c.how.k_join);
            ++bad;
            continue;
        }
        // alone, from and into exact-size allocations
        uint8_t* in = (uint8_t*)malloc(px);
        uint8_t* op = (uint8_t*)malloc(px);
        int32_t* tb = (int32_t*)malloc((size_t)(r ? r : 1) * 8 * 4);
        memcpy(in, c.px.data(), px);
        const uint8_t* ip = in;
        int cnt = -7;
        if (pseg_text_regions_host(1, &ip, &c.H, &c.W, &c.how, &op, r, r ? tb : nullptr, &cnt) != PSEG_OK) { fprintf(stderr, "case %d: the call failed: %s\n", i, pseg::last_error().c_str()); ++bad; }
        else if (memcmp(op, want.data(), px) != 0 || cnt != r || (r > 0 && memcmp(tb, rows.data(), rows.size() * 4) != 0)) { fprintf(stderr, "case %d: alone and in the list differ\n", i); ++bad; }
        // a table one row too small: the count, no row; no mask, no table
        if (r > 0) {
            int32_t* small = (int32_t*)malloc((size_t)(r > 1 ? r - 1 : 1) * 8 * 4);
            memset(small, 0x5A, (size_t)(r > 1 ? r - 1 : 1) * 8 * 4);
            cnt = -7;
            if (pseg_text_regions_host(1, &ip, &c.H, &c.W, &c.how, nullptr, r - 1, r > 1 ? small : nullptr, &cnt) != PSEG_OK || cnt != r ||
                (r > 1 && small[0] != 0x5A5A5A5A)) { fprintf(stderr, "case %d: a table of %d rows for %d regions\n", i, r - 1, r); ++bad; }
            free(small);
        }
        // the polygons, exact-size: first the needed size, then the vertices
        int64_t* first = (int64_t*)malloc((size_t)(r + 1) * 8);
        if (pseg_trace_regions_host(op, c.H, c.W, r, tb, nullptr, 0, first) != PSEG_OK) { fprintf(stderr, "case %d: the tracer failed: %s\n", i, pseg::last_error().c_str()); ++bad; }
        else {
            const int64_t need = first[r];
            int32_t* xy = (int32_t*)malloc((size_t)(need ? need : 1) * 8);
            if (pseg_trace_regions_host(op, c.H, c.W, r, tb, xy, need, first) != PSEG_OK || first[r] != need || first[0] != 0) { fprintf(stderr, "case %d: the tracer's second call failed\n", i); ++bad; }
            else {
                vertices += need;
                std::vector<int> lab;
                flood(want, c.H, c.W, lab);
                for (int k = 0; k < r; ++k) {
                    const int64_t a = first[k], b = first[k + 1];
                    long long twice = 0;
                    int x0 = 1 << 30, y0 = 1 << 30, x1 = -1, y1 = -1;
                    for (int64_t v = a; v < b; ++v) {
                        const int64_t w = v + 1 < b ? v + 1 : a;
                        twice += (long long)xy[2 * v] * xy[2 * w + 1] - (long long)xy[2 * w] * xy[2 * v + 1];
                        if (xy[2 * v] < x0) x0 = xy[2 * v];
                        if (xy[2 * v] > x1) x1 = xy[2 * v];
                        if (xy[2 * v + 1] < y0) y0 = xy[2 * v + 1];
                        if (xy[2 * v + 1] > y1) y1 = xy[2 * v + 1];
                    }
                    const int32_t* row = tb + (size_t)k * 8;
                    const bool isl = has_island(want, c.H, c.W, lab, lab[(size_t)row[5] * c.W + row[6]]);
                    islands += isl;
                    if (b - a < 4 || twice <= 0 || x0 != row[0] || y0 != row[1] || x1 != row[2] || y1 != row[3] || xy[2 * a] != row[6] || xy[2 * a + 1] != row[5] ||
                        (!isl && twice / 2 != row[4]) || (isl && twice / 2 <= row[4])) {
                        fprintf(stderr, "case %d region %d: the polygon (area %lld, clockwise %d) does not fit its row (area %d)\n", i, k, twice / 2, twice > 0, row[4]);
                        ++bad;
                    }
                }
                // the host twin of the device tracer (the word-run walk over bit planes) against the pixel walk above: the same rows,
                // offsets and vertices from exact-size arrays, then a capacity one vertex short
                int64_t* f2 = (int64_t*)malloc((size_t)(r + 1) * 8);
                int32_t* xy2 = (int32_t*)malloc((size_t)(need ? need : 1) * 8);
                int32_t* tb2 = (int32_t*)malloc((size_t)(r ? r : 1) * 8 * 4);
                int st = -7;
                cnt = -7;
                if (pseg_text_regions_poly_host(1, &ip, &c.H, &c.W, &c.how, nullptr, r, r ? tb2 : nullptr, &cnt, need ? xy2 : nullptr, need, f2, &st) != PSEG_OK ||
                    st != PSEG_OK || cnt != r || (r > 0 && memcmp(tb2, tb, (size_t)r * 8 * 4) != 0) || memcmp(f2, first, (size_t)(r + 1) * 8) != 0 ||
                    (need > 0 && memcmp(xy2, xy, (size_t)need * 8) != 0)) {
                    fprintf(stderr, "case %d: the word-run walk differs from the pixel walk: %s\n", i, pseg::last_error().c_str());
                    ++bad;
                }
                ++twins;
                if (need > 0) {
                    for (int k = 0; k <= r; ++k) f2[k] = -7;
                    int32_t* xy3 = (int32_t*)malloc((size_t)(need > 1 ? need - 1 : 1) * 8);
                    memset(xy3, 0x5A, (size_t)(need > 1 ? need - 1 : 1) * 8);
                    bool ok = pseg_text_regions_poly_host(1, &ip, &c.H, &c.W, &c.how, nullptr, r, tb2, &cnt, need > 1 ? xy3 : nullptr, need - 1, f2, &st) == PSEG_OK &&
                              st == PSEG_OK && cnt == r && f2[r] == need && xy3[0] == 0x5A5A5A5A;
                    for (int k = 0; k < r; ++k) ok = ok && f2[k] == -7;
                    if (!ok) { fprintf(stderr, "case %d: a capacity of %lld for %lld vertices\n", i, (long long)need - 1, (long long)need); ++bad; }
                    free(xy3);
                }
                free(tb2);
                free(xy2);
                free(f2);
            }
            free(xy);
        }
        free(first);
        free(tb);
        free(op);
        free(in);
    }
    printf("regions_check: %d cases against a per-pixel loop and a flood fill (%lld regions, %lld with an island, %lld vertices; the word-run walk of %lld cases "
           "against the pixel walk), %d mismatches\n", n, regions, islands, vertices, twins, bad);
    return bad ? 1 : 0;
}
