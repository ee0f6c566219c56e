// Stand-alone CPU run of the GFF3 line function (deepgrp_amd/csrc/gff_line.h, the one dgrp_gff_parse compiles for the device) for a
// sanitizer build: the text, the names table and the key sit in heap blocks of exactly their sizes, so a read one byte outside any
// of them is an error of the run, as is any undefined arithmetic.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I deepgrp_amd/csrc tools/gff_line_check.cpp -o check
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined --offload-arch=gfx950 -x hip ... builds the same host code
//   ./check TEXT TABLE [KEY]
//
// TABLE: one alternative per line, `number<TAB>bytes`, in ascending byte order (tools/gff_line_check.py writes the test corpus of
// tests/gff_in_cases.py in this form, runs this program over every case and compares what it prints with the expectations).  KEY:
// the attribute key; none = the type column.  Prints `lines rows E undecided malformed_line`, then per row
// `line begin end number name_pos name_len`.  The walk is the file-level rule on one thread: E first, then every line in front of it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "gff_line.h"

static uint8_t *slurp(const char *path, int64_t &n)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);                               // exactly n bytes: nothing behind them is ours
    if (n && fread(p, 1, n, f) != (size_t)n) { perror(path); exit(2); }
    fclose(f);
    if (n == 0) { free(p); p = nullptr; }
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s TEXT TABLE [KEY]\n", argv[0]); return 2; }
    int64_t n = 0, tn = 0;
    uint8_t *t = slurp(argv[1], n), *tb = slurp(argv[2], tn);
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> number;
    std::string blob;
    for (int64_t p = 0; p < tn;) {
        int64_t e = p;
        while (e < tn && tb[e] != '\n') ++e;
        int64_t tab = p;
        while (tab < e && tb[tab] != '\t') ++tab;
        number.push_back((int32_t)atoi(std::string((const char *)tb + p, tab - p).c_str()));
        blob.append((const char *)tb + tab + 1, e - tab - 1);
        off.push_back((int64_t)blob.size());
        p = e + 1;
    }
    free(tb);
    uint8_t *names = (uint8_t *)malloc(blob.size() ? blob.size() : 1);
    memcpy(names, blob.data(), blob.size());
    const int key_len = argc > 3 ? (int)strlen(argv[3]) : 0;
    uint8_t *key = (uint8_t *)malloc(key_len ? key_len : 1);
    if (key_len) memcpy(key, argv[3], key_len);
    const gff_table tab = { names, off.data(), number.data(), (int)number.size(), key, key_len };

    int64_t end_at = n;
    for (int64_t s = 0; s < n;) {
        if (gff_ends_features(t, s, n)) { end_at = s; break; }
        while (s < n && t[s] != '\n') ++s;
        ++s;
    }
    bool bad = false;
    for (int64_t p = 0; p < end_at; ++p) {                                   // the byte rule of rm_scan_chunk, on the text in front of E
        const uint8_t c = t[p];
        if (c == '\r' ? (p + 1 >= end_at || t[p + 1] != '\n') : !((c >= 0x20 && c <= 0x7e) || c == '\t' || c == '\n')) bad = true;
    }
    std::vector<gff_row> rows;
    std::vector<int64_t> line_of;
    int64_t lines = 0, malformed = 0;
    for (int64_t s = 0; s < end_at;) {
        ++lines;
        gff_row row;
        bool dummy = false;
        const int counted = gff_line(t, s, end_at, tab, false, row, dummy);    // the count pass, then the write pass, as on the device
        const int what = gff_line(t, s, end_at, tab, true, row, bad);
        if (counted != what) { fprintf(stderr, "line %lld: the two passes differ\n", (long long)lines); return 1; }
        if (what == GFF_SHORT && !malformed) malformed = lines;
        if (what == GFF_ROW) { rows.push_back(row); line_of.push_back(lines); }
        while (s < end_at && t[s] != '\n') ++s;
        ++s;
    }
    printf("%lld %lld %lld %d %lld\n", (long long)lines, (long long)rows.size(), (long long)end_at, bad ? 1 : 0, (long long)malformed);
    if (!bad && !malformed)
        for (size_t i = 0; i < rows.size(); ++i)
            printf("%lld %lld %lld %lld %lld %d\n", (long long)line_of[i], (long long)rows[i].begin, (long long)rows[i].end,
                   (long long)rows[i].number, (long long)rows[i].name_pos, rows[i].name_len);
    free(t);
    free(names);
    free(key);
    return 0;
}
