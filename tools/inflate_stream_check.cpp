// Stand-alone check of the host side of the plain-gzip path (deepgrp_amd/csrc/inflate_stream.h) and of the member path
// (dgrp_inflate_core of inflate.h, what dgrp_inflate_raw_host runs) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/inflate_stream_check.cpp -o check
//   ./check STREAM [STREAM ...]
//
// Every STREAM is a file of raw DEFLATE data; beside a valid one lies STREAM.txt with the text it inflates to (a stream without it
// is expected to be refused or to fit into 4 MiB).  Each is inflated as one member and at chunk sizes of 1, 4 and 32 KiB into a heap buffer of exactly
// the text's size, so a write outside it is the sanitizer's to report.  Exit status 1 when a text differs.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../deepgrp_amd/csrc/inflate_stream.h"

static bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

int main(int argc, char **argv)
{
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> comp, want;
        if (!slurp(argv[a], comp)) {
            fprintf(stderr, "%s: cannot read\n", argv[a]);
            return 2;
        }
        const bool valid = slurp(std::string(argv[a]) + ".txt", want);
        const int64_t cap = valid ? (int64_t)want.size() : 4 << 20;
        {                                                            // the member path: the same block loop, no window
            uint8_t *out = new uint8_t[(size_t)cap];
            uint8_t *in = new uint8_t[comp.size()];
            if (!comp.empty()) memcpy(in, comp.data(), comp.size());
            dgrp_inflate_tables t;
            dgrp_host_sink sink{out};
            uint32_t out_len = 0, in_used = 0;
            const int rc = dgrp_inflate_core(in, (uint32_t)comp.size(), (uint32_t)cap, &t, sink, &out_len, &in_used);
            const bool same = rc == DGRP_INFLATE_OK && out_len == cap && (cap == 0 || memcmp(out, want.data(), (size_t)cap) == 0);
            printf("%s member path: reason %d, %u bytes, %u of %zu input bytes used%s\n", argv[a], rc, out_len, in_used, comp.size(),
                   valid ? (same ? ", equal" : ", DIFFERENT") : "");
            if (valid && !same) bad = 1;
            delete[] out;
            delete[] in;
        }
        for (int64_t chunk : {1 << 10, 4 << 10, 32 << 10}) {
            uint8_t *out = new uint8_t[(size_t)cap];
            uint8_t *in = new uint8_t[comp.size()];                  // exactly sized as well: a read past the stream shows
            if (!comp.empty()) memcpy(in, comp.data(), comp.size());
            int64_t out_len = 0, in_used = 0;
            int reason = 0;
            dgrp_inflate_stream_stats st = {};
            const int rc = dgrp_stream_inflate_host(in, (int64_t)comp.size(), chunk, 1 << 22, 64, out, cap, &out_len, &in_used, &st, &reason);
            const bool same = rc == DGRP_OK && out_len == cap && (cap == 0 || memcmp(out, want.data(), (size_t)cap) == 0);
            printf("%s chunk %lld: rc %d reason %d, %lld bytes, %lld spans, %lld rounds%s\n", argv[a], (long long)chunk, rc, reason,
                   (long long)out_len, (long long)st.spans, (long long)st.rounds, valid ? (same ? ", equal" : ", DIFFERENT") : "");
            if (valid && !same) bad = 1;
            delete[] out;
            delete[] in;
        }
    }
    return bad;
}
