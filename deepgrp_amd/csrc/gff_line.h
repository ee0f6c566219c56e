// One line of GFF3 -> one row: the line function of dgrp_gff_parse (gff_parse_kernels.hip), on its own so that a CPU program can run
// it over a corpus under a sanitizer (tools/gff_line_check.cpp).  The grammar is stated in include/deepgrp_hip.h (dgrp_gff_parse) and,
// as Python, in deepgrp_amd/gffin.py.  Bytes and integers only; nothing is written to the text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GFF_HD __host__ __device__
#else
#define GFF_HD
#endif

#define GFF_MIN_LINE 11                  // shortest feature line: eight tabs, one digit each for start and end, and the line feed
#define GFF_MAX_DIGITS 18                // a coordinate of more digits is left to the host
#define GFF_MAX_NAMES 4096               // alternatives of the names table
#define GFF_MAX_KEY 255                  // bytes of the attribute key

enum { GFF_SKIP = 0, GFF_ROW = 1, GFF_SHORT = 2 };

struct gff_row {
    int64_t begin, end, number, name_pos;
    int32_t name_len;
};

// What a label string is looked up in and where it is taken from: `nnames` alternatives names[off[k] .. off[k + 1]) in ascending byte
// order (a proper prefix first), number[k] the number of alternative k; the attribute key, key_len == 0 for the type column.
struct gff_table {
    const uint8_t *names;
    const int64_t *off;
    const int32_t *number;
    int nnames;
    const uint8_t *key;
    int key_len;
};

GFF_HD inline bool gff_eol(uint8_t c) { return c == '\n' || c == '\r'; }

GFF_HD inline int gff_hex(uint8_t c)
{
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// Whether the line that starts at s ends the features: exactly `##FASTA` (a carriage return directly before the line feed belongs
// to the line end), or a first byte '>'.
GFF_HD inline bool gff_ends_features(const uint8_t *__restrict__ t, int64_t s, int64_t n)
{
    if (s >= n) return false;
    if (t[s] == '>') return true;
    if (n - s < 7) return false;
    const char *word = "##FASTA";
    for (int j = 0; j < 7; ++j)
        if (t[s + j] != (uint8_t)word[j]) return false;
    if (s + 7 == n || t[s + 7] == '\n') return true;
    return t[s + 7] == '\r' && s + 8 < n && t[s + 8] == '\n';
}

// [b, e) as 1..18 plain decimal digits, else `bad`
GFF_HD inline int64_t gff_number(const uint8_t *__restrict__ t, int64_t b, int64_t e, bool &bad)
{
    if (e - b < 1 || e - b > GFF_MAX_DIGITS) { bad = true; return 0; }
    int64_t val = 0;
    for (int64_t p = b; p < e; ++p) {
        const uint8_t c = t[p];
        if (c < '0' || c > '9') { bad = true; return 0; }
        val = val * 10 + (c - '0');
    }
    return val;
}

// t[b, e) with its %XX decoded against name[0, len): < 0, 0, > 0 as memcmp orders them, a proper prefix first.  '%' and two hex digits
// of either case inside the span are that byte, any other '%' is itself.
GFF_HD inline int gff_compare_decoded(const uint8_t *__restrict__ t, int64_t b, int64_t e, const uint8_t *__restrict__ name, int64_t len)
{
    int64_t j = 0;
    for (int64_t p = b; p < e; ++j) {
        int c = t[p];
        int hi, lo;
        if (c == '%' && e - p >= 3 && (hi = gff_hex(t[p + 1])) >= 0 && (lo = gff_hex(t[p + 2])) >= 0) {
            c = hi * 16 + lo;
            p += 3;
        } else {
            ++p;
        }
        if (j >= len) return 1;                                              // the alternative is a proper prefix
        if (c != (int)name[j]) return c < (int)name[j] ? -1 : 1;
    }
    return j < len ? -1 : 0;
}

// The number of the alternative byte-equal to the decoded t[b, e), 0 where there is none: a binary search, which stays inside the
// table whatever its order.
GFF_HD inline int64_t gff_lookup(const uint8_t *__restrict__ t, int64_t b, int64_t e, const gff_table &tab)
{
    int lo = 0, hi = tab.nnames;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const int64_t o = tab.off[mid];
        const int c = gff_compare_decoded(t, b, e, tab.names + o, tab.off[mid + 1] - o);
        if (c == 0) return (int64_t)tab.number[mid];
        if (c < 0) hi = mid; else lo = mid + 1;
    }
    return 0;
}

// The value of the first piece of the attribute column t[b, e) whose tag is byte-equal to the key: pieces between ';', a piece cut at
// its first '='.  -> false where no piece has the key.
GFF_HD inline bool gff_attribute(const uint8_t *__restrict__ t, int64_t b, int64_t e, const uint8_t *__restrict__ key, int key_len,
                                 int64_t &vb, int64_t &ve)
{
    int64_t pb = b;
    while (pb <= e) {
        int64_t pe = pb, eq = -1;
        for (; pe < e && t[pe] != ';'; ++pe)
            if (eq < 0 && t[pe] == '=') eq = pe;
        if (eq >= 0 && eq - pb == key_len) {
            bool same = true;
            for (int j = 0; same && j < key_len; ++j) same = t[pb + j] == key[j];
            if (same) { vb = eq + 1; ve = pe; return true; }
        }
        pb = pe + 1;
    }
    return false;
}

// The line that starts at s, in a text of n bytes: empty, or a first byte '#': skipped; fewer than nine fields between single tabs:
// short; else a row -- field 1 the name, fields 4 and 5 start and end (begin = start - 1), and with `numbered` the number of its label
// string (field 3, or the value of the key in field 9, which runs to the line end).
GFF_HD inline int gff_line(const uint8_t *__restrict__ t, int64_t s, int64_t n, const gff_table &tab, bool numbered, gff_row &row, bool &bad)
{
    int64_t tab_at[8], p = s;
    int tabs = 0;
    for (; p < n && !gff_eol(t[p]); ++p)
        if (t[p] == '\t' && tabs < 8) tab_at[tabs++] = p;
    const int64_t e = p;
    if (e == s || t[s] == '#') return GFF_SKIP;
    if (tabs < 8) return GFF_SHORT;
    row.begin = gff_number(t, tab_at[2] + 1, tab_at[3], bad) - 1;
    row.end = gff_number(t, tab_at[3] + 1, tab_at[4], bad);
    if (tab_at[0] - s > 0x7fffffffll) bad = true;                            // (a name the int32 length cannot state)
    row.name_pos = s;
    row.name_len = (int32_t)(tab_at[0] - s);
    row.number = 0;
    if (numbered && tab.nnames > 0) {
        int64_t vb = tab_at[1] + 1, ve = tab_at[2];
        if (tab.key_len == 0 || gff_attribute(t, tab_at[7] + 1, e, tab.key, tab.key_len, vb, ve)) row.number = gff_lookup(t, vb, ve, tab);
    }
    return GFF_ROW;
}
