// Stand-alone CPU restatement of the probe / compare loop of dgrp_token_ids (deepgrp_amd/csrc/offtarget_kernels.hip) for a sanitizer
// build -- the device code itself is not compiled here; what is checked is the protocol: that ids are exact whatever the hash and
// whichever thread claims a slot first.
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/token_table_check.cpp -o check && ./check
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=thread tools/token_table_check.cpp -o check_t && ./check_t
//
// Tokens are one or two spans of a text (the logical string `a` or `a/b`, never joined), as the parser hands them over.  Eight threads
// insert interleaved stripes of the rows into a table of 65 536 atomic 64-bit words -- EMPTY or the row that claimed the slot with one
// compare-and-swap; a row that meets a taken slot compares its own bytes with the claimant's and takes the slot when they are equal,
// else probes on.  Run with the real hash (FNV-1a), with a hash of 3 bits and with a constant hash: every row's slot must hold a
// claimant of ITS string, no two slots the same string, and the ranks of the slots' strings must equal the ranks of a std::set.
// Exit status 1 when anything differs.
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

static const uint32_t SLOTS = 65536;
static const uint64_t EMPTY = ~0ull;

struct Row {
    int64_t a, b;
    int32_t la, lb;                      // lb = 0: the first span alone
    int64_t len() const { return (int64_t)la + (lb > 0 ? 1 + (int64_t)lb : 0); }
    uint8_t at(const std::vector<uint8_t> &t, int64_t j) const { return j < la ? t[a + j] : (j == la ? (uint8_t)'/' : t[b + (j - la - 1)]); }
};

static uint64_t hash_of(const std::vector<uint8_t> &t, const Row &s, int mode)
{
    if (mode == 2) return 0;
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t j = 0; j < s.len(); ++j) h = (h ^ s.at(t, j)) * 0x100000001b3ull;
    h ^= h >> 32;
    return mode == 1 ? (h & 7) : h;
}

static int32_t insert(const std::vector<uint8_t> &t, const std::vector<Row> &rows, std::vector<std::atomic<uint64_t>> &table, int64_t i, int mode)
{
    const Row &s = rows[i];
    const int64_t L = s.len();
    uint32_t slot = (uint32_t)hash_of(t, s, mode) & (SLOTS - 1);
    for (uint32_t probe = 0; probe < SLOTS; ++probe, slot = (slot + 1) & (SLOTS - 1)) {
        uint64_t owner = table[slot].load(std::memory_order_relaxed);
        if (owner == EMPTY) {
            uint64_t expect = EMPTY;
            owner = table[slot].compare_exchange_strong(expect, (uint64_t)i, std::memory_order_relaxed) ? EMPTY : expect;
        }
        if (owner == EMPTY) return (int32_t)slot;
        const Row &o = rows[owner];
        bool same = o.len() == L;
        for (int64_t j = 0; same && j < L; ++j) same = o.at(t, j) == s.at(t, j);
        if (same) return (int32_t)slot;
    }
    return -1;
}

static std::string logical(const std::vector<uint8_t> &t, const Row &s)
{
    std::string out;
    for (int64_t j = 0; j < s.len(); ++j) out.push_back((char)s.at(t, j));
    return out;
}

int main()
{
    // the text: tokens with shared prefixes, tokens that differ in the last byte, 1-byte tokens, and both spellings of one string
    std::vector<std::string> words;
    for (int k = 0; k < 3000; ++k) words.push_back("LTR/ERV" + std::to_string(k % 1500));
    for (const char *w : { "L", "LT", "LTR", "LTR/", "LINE/L2", "LINE/L", "LINE", "/", "a", "b", "DNA/hAT", "DNA/hAT-Charlie" }) words.push_back(w);
    std::vector<uint8_t> text;
    std::vector<Row> rows;
    for (size_t k = 0; k < words.size(); ++k) {
        const std::string &w = words[k];
        const size_t cut = w.find('/');
        Row r = { (int64_t)text.size(), 0, (int32_t)w.size(), 0 };
        if (k % 2 == 1 && cut != std::string::npos && cut + 1 < w.size() && cut > 0) {      // the two-span spelling
            r.la = (int32_t)cut;
            text.insert(text.end(), w.begin(), w.begin() + cut);
            text.push_back('\t');
            r.b = (int64_t)text.size();
            r.lb = (int32_t)(w.size() - cut - 1);
            text.insert(text.end(), w.begin() + cut + 1, w.end());
        } else {
            text.insert(text.end(), w.begin(), w.end());
        }
        text.push_back(' ');
        rows.push_back(r);
    }
    std::set<std::string> distinct(words.begin(), words.end());
    std::map<std::string, int> want;
    for (const std::string &w : distinct) want.emplace(w, (int)want.size());
    int bad = 0;
    for (int mode = 0; mode < 3; ++mode) {
        std::vector<std::atomic<uint64_t>> table(SLOTS);
        for (auto &w : table) w.store(EMPTY, std::memory_order_relaxed);
        std::vector<int32_t> slot_of(rows.size(), -2);
        const int T = 8;
        std::vector<std::thread> pool;
        for (int th = 0; th < T; ++th)
            pool.emplace_back([&, th] {
                for (size_t i = th; i < rows.size(); i += T) slot_of[i] = insert(text, rows, table, (int64_t)i, mode);
            });
        for (auto &th : pool) th.join();
        // the occupied slots in slot order, their strings, the ranks
        std::vector<std::string> held;
        std::vector<int> comp(SLOTS, -1);
        for (uint32_t s = 0; s < SLOTS; ++s) {
            const uint64_t owner = table[s].load();
            if (owner == EMPTY) continue;
            comp[s] = (int)held.size();
            held.push_back(logical(text, rows[owner]));
        }
        std::set<std::string> once(held.begin(), held.end());
        if (held.size() != distinct.size() || once.size() != held.size()) {
            printf("mode %d: %zu slots for %zu distinct tokens (%zu distinct among the slots)\n", mode, held.size(), distinct.size(), once.size());
            ++bad;
        }
        for (size_t i = 0; i < rows.size(); ++i) {
            if (slot_of[i] < 0 || comp[slot_of[i]] < 0 || held[comp[slot_of[i]]] != words[i] || want[held[comp[slot_of[i]]]] != want[words[i]]) {
                printf("mode %d: row %zu (%s) sits in slot %d\n", mode, i, words[i].c_str(), slot_of[i]);
                ++bad;
                break;
            }
        }
        printf("mode %d: %zu rows, %zu distinct tokens, %s\n", mode, rows.size(), held.size(), bad ? "WRONG" : "exact");
    }
    return bad ? 1 : 0;
}
