// pngdec_check -- the PNG reader's host entry under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
// (csrc/Makefile: make pngdec_check).  It reads a corpus directory written by tools/pngdec_corpus.py -- <name>.png, and next to
// it <name>.expect holding the status and, for a file that decodes, the H * W gray bytes PIL gives -- and runs the whole list
// through pseg_png_decode_gray_host in one call, then every file alone with its output placed at the end of an exact-size
// allocation, so that a write past H * W bytes is caught.  Exit status 0: every status and every byte as expected.
#include <dirent.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pseg.h"

namespace pseg {                                   // what pseg_pngdec.hip takes from pseg_engine.hip in the library
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

static std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CORPUS_DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::vector<std::string> names;
    DIR* d = opendir(dir.c_str());
    if (!d) { fprintf(stderr, "cannot open %s\n", dir.c_str()); return 2; }
    while (dirent* e = readdir(d)) {
        const std::string n = e->d_name;
        if (n.size() > 4 && n.substr(n.size() - 4) == ".png") names.push_back(n.substr(0, n.size() - 4));
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    const int n = (int)names.size();
    if (n == 0) { fprintf(stderr, "empty corpus\n"); return 2; }
    std::vector<std::vector<uint8_t>> files(n), want(n);
    std::vector<int> want_st(n), Hs(n), Ws(n);
    for (int i = 0; i < n; ++i) {
        files[i] = slurp(dir + "/" + names[i] + ".png");
        std::vector<uint8_t> e = slurp(dir + "/" + names[i] + ".expect");   // "<status> <H> <W>\n" then the gray bytes
        const size_t nl = std::find(e.begin(), e.end(), (uint8_t)'\n') - e.begin();
        if (nl == e.size() || sscanf(std::string(e.begin(), e.begin() + nl).c_str(), "%d %d %d", &want_st[i], &Hs[i], &Ws[i]) != 3) {
            fprintf(stderr, "%s.expect: bad header\n", names[i].c_str());
            return 2;
        }
        want[i].assign(e.begin() + nl + 1, e.end());
    }
    int bad = 0;
    auto check = [&](int i, int st, const uint8_t* out, const char* how) {
        if (st != want_st[i]) { fprintf(stderr, "%s (%s): status %d, expected %d\n", names[i].c_str(), how, st, want_st[i]); ++bad; return; }
        if (st == PSEG_OK) {
            if (want[i].size() != (size_t)Hs[i] * Ws[i] || memcmp(out, want[i].data(), want[i].size()) != 0) { fprintf(stderr, "%s (%s): pixels differ\n", names[i].c_str(), how); ++bad; }
        } else {
            for (size_t k = 0; k < (size_t)Hs[i] * Ws[i]; ++k)
                if (out[k] != 0xA5) { fprintf(stderr, "%s (%s): a refused file's output was written\n", names[i].c_str(), how); ++bad; break; }
        }
    };
    // the whole list in one call
    {
        std::vector<uint8_t*> outs(n);
        std::vector<const uint8_t*> ptrs(n);
        std::vector<size_t> lens(n);
        std::vector<int> st(n, 7);
        for (int i = 0; i < n; ++i) {
            outs[i] = (uint8_t*)malloc((size_t)Hs[i] * Ws[i] + 1);
            memset(outs[i], 0xA5, (size_t)Hs[i] * Ws[i] + 1);
            ptrs[i] = files[i].data();
            lens[i] = files[i].size();
        }
        if (pseg_png_decode_gray_host(n, ptrs.data(), lens.data(), outs.data(), st.data()) != PSEG_OK) { fprintf(stderr, "the list call failed: %s\n", pseg::last_error().c_str()); return 1; }
        for (int i = 0; i < n; ++i) { check(i, st[i], outs[i], "list"); free(outs[i]); }
    }
    // every file alone, from an exact-size copy (a read past its end is caught) into an exact-size output
    for (int i = 0; i < n; ++i) {
        const size_t nb = files[i].size(), no = (size_t)Hs[i] * Ws[i];
        uint8_t* f = (uint8_t*)malloc(nb ? nb : 1);
        memcpy(f, files[i].data(), nb);
        uint8_t* out = (uint8_t*)malloc(no ? no : 1);
        memset(out, 0xA5, no);
        const uint8_t* fp = f;
        int st = 7;
        if (pseg_png_decode_gray_host(1, &fp, &nb, &out, &st) != PSEG_OK) { fprintf(stderr, "%s: the call failed\n", names[i].c_str()); ++bad; }
        else check(i, st, out, "alone");
        free(out);
        free(f);
    }
    printf("pngdec_check: %d files, %d mismatches\n", n, bad);
    return bad ? 1 : 0;
}
