// emu_spread_cut.cpp — k_spread_cut (swarmkit_amd/csrc/swp_scan_spread.hpp: where a compact spread segment that is too wide is cut)
// on CPU fibers against a sequential bitset model of the rule. TEST INFRASTRUCTURE; no GPU.
//
//   emu_spread_cut <case> [g]        g: the piece's union in global memory (cu) instead of LDS
//
// A case is a set of class rows over N nodes, a segment of tasks (class row, has preferences), a limit L and a piece list of
// max_pieces. Compared word for word: the status, the task an own row is reported for, the piece list, the number of counts the
// kernel made (a task whose row the piece holds already must not cost one), and that nothing behind the list was written. The
// events a case is named for are printed for the Python side to assert (tests/test_emu_spread_cut.py).
#include <set>
#include <string>
#include <vector>

#include "wv_emu.hpp"

#define SWP_R6_KERNELS
#include "../../swarmkit_amd/csrc/swp_resolve6.hpp"
#define SWP_SCAN_SPREAD_KERNEL
#include "../../swarmkit_amd/csrc/swp_scan_spread.hpp"

using namespace swpdev;

struct Case {
    u32 N = 0, L = 0, max_pieces = 0, j0 = 0;
    std::vector<std::vector<u64>> rows;
    std::vector<u32> sc, pref;   // per task of the batch (the segment is [j0, sc.size()))
    u32 words() const { return (N + 63) / 64; }
    u32 row_range(u32 a, u32 b) {   // the nodes [a, b)
        std::vector<u64> r(words(), 0);
        for (u32 n = a; n < b && n < N; ++n) r[n >> 6] |= 1ull << (n & 63);
        rows.push_back(r);
        return (u32)rows.size() - 1;
    }
    void task(u32 row, bool p, u32 times = 1) {
        for (u32 i = 0; i < times; ++i) { sc.push_back(row); pref.push_back(p ? 7u : 0u); }   // (any non-zero word means preferences)
    }
};

struct Result {
    u32 status = CUT_OK, bad = 0, counts = 0;
    std::vector<u32> pieces;   // (first, count, spread)
    u32 cut_plain = 0, cut_pref = 0, again = 0, rode = 0, at_limit = 0, over_by_one = 0;
};

static u32 popc_or(const std::vector<u64>& a, const std::vector<u64>& b) {
    u32 c = 0;
    for (size_t w = 0; w < a.size(); ++w) c += (u32)__builtin_popcountll(a[w] | b[w]);
    return c;
}

// the rule, one task after the other
static Result model(const Case& c) {
    Result r;
    const u32 j1 = (u32)c.sc.size();
    std::set<u32> ever;
    auto emit = [&](u32 first, u32 n, u32 spread) {
        if (r.pieces.size() / 3 == c.max_pieces) { r.status = CUT_FULL; return false; }
        r.pieces.push_back(first); r.pieces.push_back(n); r.pieces.push_back(spread);
        return true;
    };
    const std::vector<u64> none(c.words(), 0);
    for (u32 j = c.j0; j < j1;) {
        std::vector<u64> U = c.rows[c.sc[j]];
        std::set<u32> in{c.sc[j]};
        ++r.counts;
        if (ever.count(c.sc[j])) ++r.again;
        if (popc_or(U, none) > c.L) { r.status = CUT_OWN_ROW; r.bad = j; return r; }
        u32 k = j + 1;
        for (; k < j1; ++k) {
            if (in.count(c.sc[k])) { ++r.rode; continue; }
            ++r.counts;
            const u32 n = popc_or(U, c.rows[c.sc[k]]);
            if (n == c.L) ++r.at_limit;
            if (n == c.L + 1) ++r.over_by_one;
            if (n > c.L) break;
            for (size_t w = 0; w < U.size(); ++w) U[w] |= c.rows[c.sc[k]][w];
            in.insert(c.sc[k]);
            if (ever.count(c.sc[k])) ++r.again;
        }
        if (!emit(j, k - j, 1)) return r;
        ever.insert(in.begin(), in.end());
        if (k == j1) break;
        if (c.pref[k]) { ++r.cut_pref; j = k; continue; }
        ++r.cut_plain;
        u32 p = k + 1;
        while (p < j1 && !c.pref[p]) ++p;
        if (!emit(k, p - k, 0)) return r;
        j = p;
    }
    return r;
}

static u64 rng_state = 1;
static u32 rnd() {
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (u32)((rng_state * 0x2545F4914F6CDD1Dull) >> 33);
}

// rows of random width around a few centres, tasks that name rows near a base that moves on: pieces of some dozen tasks
static Case random_case(u64 seed, u32 N, u32 n_sc, u32 T, u32 L, u32 j0) {
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    Case c;
    c.N = N; c.L = L; c.max_pieces = T; c.j0 = j0;
    for (u32 i = 0; i < n_sc; ++i) {
        const u32 len = 1 + rnd() % (rnd() % 9 == 0 ? L + L / 8 : L / 2 + 1), a = rnd() % N;
        const u32 row = c.row_range(a, a + len);
        for (u32 s = rnd() % 4; s; --s) { const u32 n = rnd() % N; c.rows[row][n >> 6] |= 1ull << (n & 63); }
        if (rnd() % 41 == 0) c.rows[row] = std::vector<u64>(c.words(), 0);   // (an empty row fits anywhere)
    }
    u32 base = 0;
    for (u32 t = 0; t < T; ++t) {
        if (rnd() % 23 == 0) base = rnd() % n_sc;
        c.sc.push_back((base + rnd() % 3) % n_sc);
        c.pref.push_back(t == j0 || rnd() % 5 < 3 ? 1u + rnd() % 9 : 0u);
    }
    // the segment's first task has preferences and a row of its own that fits
    const std::vector<u64> none(c.words(), 0);
    while (popc_or(c.rows[c.sc[j0]], none) > L) c.sc[j0] = (c.sc[j0] + 1) % n_sc;
    for (u32 t = j0 + 1; t < T; ++t)   // (a row beyond the limit is a plain task's: the own-row refusal has cases of its own)
        if (popc_or(c.rows[c.sc[t]], none) > L) c.pref[t] = 0;
    return c;
}

static Case make_case(const std::string& name) {
    Case c;
    c.N = 4097; c.L = 100; c.max_pieces = 64;
    if (name == "nocut") {
        const u32 a = c.row_range(0, 40), b = c.row_range(20, 60);
        c.task(a, true); c.task(b, false); c.task(a, true, 2); c.task(b, true); c.task(a, false);
    } else if (name == "plain_cut") {   // an unconstrained plain task rides along: spread, plain, spread
        const u32 a = c.row_range(4000, 4050), all = c.row_range(0, c.N);
        c.task(a, true, 3); c.task(all, false, 2); c.task(a, true, 3);
    } else if (name == "pref_cut") {   // two pools that each fit: two spread pieces, nothing between them
        const u32 a = c.row_range(0, 80), b = c.row_range(80, 160);
        c.task(a, true, 3); c.task(b, true, 3);
    } else if (name == "exact_L") {
        const u32 a = c.row_range(0, 60), b = c.row_range(60, 100);
        c.task(a, true, 2); c.task(b, true, 2); c.task(a, false);
    } else if (name == "L_plus_1") {
        const u32 a = c.row_range(0, 60), b = c.row_range(60, 101);
        c.task(a, true, 2); c.task(b, true, 2); c.task(a, false);
    } else if (name == "row_again") {   // a row seen again behind a cut counts afresh
        const u32 a = c.row_range(0, 80), b = c.row_range(80, 160);
        c.task(a, true); c.task(b, true); c.task(a, true, 2); c.task(b, false); c.task(a, true);
    } else if (name == "own_row") {
        const u32 a = c.row_range(0, 50), w = c.row_range(1000, 1101);
        c.task(a, true, 2); c.task(a, false); c.task(w, true); c.task(a, true);
    } else if (name == "own_row_first") {
        const u32 a = c.row_range(0, 50), w = c.row_range(1000, 1101);
        c.j0 = 3;
        c.task(a, false, 3); c.task(w, true); c.task(a, true);
    } else if (name == "plain_wide_row") {   // a plain task's own row beyond L is no refusal: it goes to the other resolver
        const u32 a = c.row_range(0, 50), w = c.row_range(1000, 1101);
        c.task(a, true, 2); c.task(w, false); c.task(a, false); c.task(a, true);
    } else if (name == "full") {
        const u32 a = c.row_range(0, 80), b = c.row_range(80, 160);
        c.max_pieces = 3;
        for (int i = 0; i < 4; ++i) { c.task(a, true); c.task(b, true); }
    } else if (name == "full_exact") {   // as many pieces as the list holds: not full
        const u32 a = c.row_range(0, 80), b = c.row_range(80, 160);
        c.max_pieces = 4;
        for (int i = 0; i < 2; ++i) { c.task(a, true); c.task(b, true); }
    } else if (name == "boundary") {   // more tasks than a workgroup has threads: a cut at task 1024, one at 2047, a piece start at 2049
        const u32 a = c.row_range(0, 80), a2 = c.row_range(10, 30), b = c.row_range(2000, 2090), all = c.row_range(0, c.N);
        c.j0 = 0;
        for (u32 t = 0; t < 1024; ++t) c.task(t % 3 ? a : a2, t % 4 != 1);
        for (u32 t = 1024; t < 2047; ++t) c.task(b, t == 1024 || t % 5 == 0);
        c.task(all, false, 2);
        for (u32 t = 2049; t < 2500; ++t) c.task(t % 2 ? a : a2, t == 2049 || t % 7 == 0);
    } else if (name == "boundary_j0") {   // the same segment behind 37 tasks of the batch: the chunks do not start at multiples of 1024
        Case d = make_case("boundary");
        c = d;
        c.sc.clear(); c.pref.clear();
        c.j0 = 37;
        c.task(3, false, 37);
        c.sc.insert(c.sc.end(), d.sc.begin(), d.sc.end());
        c.pref.insert(c.pref.end(), d.pref.begin(), d.pref.end());
    } else if (name == "nsc1") {
        const u32 a = c.row_range(5, 105);
        c.task(a, true); c.task(a, false, 70); c.task(a, true, 5);
    } else if (name == "nsc65") c = random_case(65, 4097, 65, 700, 100, 0);
    else if (name == "nsc300") c = random_case(300, 9000, 300, 2600, 333, 11);
    else if (name == "n9000") c = random_case(9, 9000, 40, 1500, 4096, 0);
    else if (name == "n70000") c = random_case(70, 70000, 30, 300, 2000, 0);   // more words than threads
    else { fprintf(stderr, "unknown case %s\n", name.c_str()); exit(2); }
    return c;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: emu_spread_cut <case> [g]\n"); return 2; }
    const std::string name = argv[1];
    const bool in_global = argc > 2 && argv[2][0] == 'g';
    Case c = make_case(name);
    const u32 T = (u32)c.sc.size(), Wn = c.words(), n_sc = (u32)c.rows.size();
    const Result want = model(c);

    std::vector<RTask> rt(T);
    for (u32 t = 0; t < T; ++t) { memset(&rt[t], 0, sizeof(RTask)); rt[t].sc = c.sc[t]; }
    std::vector<u64> sc((size_t)n_sc * Wn);
    for (u32 r = 0; r < n_sc; ++r) memcpy(&sc[(size_t)r * Wn], c.rows[r].data(), (size_t)Wn * 8);
    const u32 GUARD = 16, POISON = 0xEEEEEEEEu;
    std::vector<u32> out(CUT_HEAD + (size_t)3 * c.max_pieces + GUARD, POISON);
    std::vector<u64> cu(Wn + 1, 0xABABABABABABABABull);
    CutArgs a{};
    a.rt = rt.data(); a.pref = c.pref.data(); a.sc = sc.data(); a.cu = cu.data(); a.out = out.data();
    a.j0 = c.j0; a.j1 = T; a.n_sc = n_sc; a.n_words = Wn; a.L = c.L; a.max_pieces = c.max_pieces;
    a.u_lds = in_global ? 0u : 1u;
    emu::launch(SCAN_THREADS, spread_cut_lds(n_sc, Wn, !in_global), [&] { k_spread_cut(a); });

    int bad = 0;
    auto fail = [&](const char* what, unsigned long long got, unsigned long long exp) { fprintf(stderr, "MISMATCH %s: kernel %llu, model %llu\n", what, got, exp); ++bad; };
    if (out[0] != want.status) fail("status", out[0], want.status);
    if (out[1] != want.bad) fail("task", out[1], want.bad);
    if (out[2] != want.pieces.size() / 3) fail("pieces", out[2], want.pieces.size() / 3);
    if (out[3] != want.counts) fail("counts", out[3], want.counts);
    for (size_t i = 0; i < want.pieces.size(); ++i)
        if (out[CUT_HEAD + i] != want.pieces[i]) { fail("piece word", out[CUT_HEAD + i], want.pieces[i]); fprintf(stderr, "  (word %zu of piece %zu)\n", i % 3, i / 3); break; }
    for (size_t i = CUT_HEAD + want.pieces.size(); i < out.size(); ++i)
        if (out[i] != POISON) { fail("a word behind the list", out[i], POISON); break; }
    if (cu[Wn] != 0xABABABABABABABABull) fail("the word behind cu", cu[Wn], 0xABABABABABABABABull);
    if (!in_global && cu[0] != 0xABABABABABABABABull) fail("cu written although the union is in LDS", cu[0], 0);
    if (want.status == CUT_OK) {   // the pieces tile the segment
        u32 at = c.j0;
        for (size_t i = 0; i < want.pieces.size(); i += 3) { if (want.pieces[i] != at) fail("tiling", want.pieces[i], at); at += want.pieces[i + 1]; }
        if (at != T) fail("tiling end", at, T);
    }
    fprintf(stderr, "case %s: N %u words %u n_sc %u tasks [%u, %u) L %u list %u union in %s\n", name.c_str(), c.N, Wn, n_sc, c.j0, T, c.L, c.max_pieces, in_global ? "global" : "lds");
    fprintf(stderr, "status %u task %u | pieces %zu | cuts at a plain task %u | cuts at a task with preferences %u | rows counted again %u | rode along %u | counts %u | at the limit %u | one over %u\n",
            want.status, want.bad, want.pieces.size() / 3, want.cut_plain, want.cut_pref, want.again, want.rode, want.counts, want.at_limit, want.over_by_one);
    fprintf(stderr, "list:");
    for (size_t i = 0; i < want.pieces.size() && i < 3 * 12; i += 3) fprintf(stderr, " (%u,%u,%u)", out[CUT_HEAD + i], out[CUT_HEAD + i + 1], out[CUT_HEAD + i + 2]);
    fprintf(stderr, "\n-> %s\n", bad ? "FAILED" : "OK");
    return bad ? 1 : 0;
}
