// The speaker roster (csrc/roster.cpp: sd_roster_*, sd_relabel_turns_map) for AddressSanitizer + UBSan.  CPU only; tools/sanitize/build_roster.sh builds it
// together with roster.cpp itself, whose every allocation goes through roster_alloc_hook.
//   roster [seed]   rosters through random sequences of updates -- with and without row labels, shifts past the previous table, NaN rows, duplicated and
//                   zero-norm centroids, bad arguments, loaded entries -- against a second, naive implementation of the rule on std::vector (tables
//                   instead of sorted codes, repeated arg-min instead of sorted pairs).  Before every call that may allocate, the call is made with its
//                   first, second, ... allocation failing until one goes through: each failure returns SD_ERR_NOMEM and leaves the roster's content
//                   unchanged, as do SD_ERR_ARG and SD_ERR_NUMERIC.
//                   -> "roster ok: ..." and exit 0, or the first mismatch
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "roster.h"

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); fflush(stdout); return 1; } } while (0)

static long g_allocs = 0, g_fail_in = -1;      // g_fail_in >= 0: the allocation that many allocations from now fails
static void* test_alloc(size_t bytes)
{
    if (g_fail_in == 0) { g_fail_in = -1; return nullptr; }
    if (g_fail_in > 0) --g_fail_in;
    ++g_allocs;
    return malloc(bytes);      // exactly the bytes asked for: a byte past them is a report
}

// ---- the naive implementation
struct Naive { int d = 0; std::vector<std::vector<double>> cen; std::vector<int64_t> n, seen; int64_t U = 0; };

static bool nan_row(const double* x) { return x[0] != x[0]; }

static int naive_update(Naive& r, const double* C, const int64_t* m, int64_t K, const int32_t* rows, int64_t M, const int32_t* prev, int64_t Mp, int64_t shift,
                        double t, std::vector<int32_t>& ids)
{
    const int d = r.d;
    const int64_t P = (int64_t)r.n.size();
    ids.assign((size_t)K, -1);
    std::vector<char> given((size_t)P, 0);
    if (rows && prev) {
        std::vector<std::vector<int64_t>> cnt((size_t)K, std::vector<int64_t>((size_t)P, 0));
        for (int64_t i = 0; i < M; ++i) if (i + shift < Mp && rows[i] >= 0 && prev[i + shift] >= 0) cnt[(size_t)rows[i]][(size_t)prev[i + shift]]++;
        for (;;) {
            int64_t bk = -1, bp = -1;
            for (int64_t k = 0; k < K; ++k) for (int64_t p = 0; p < P; ++p)
                if (ids[(size_t)k] < 0 && !given[(size_t)p] && cnt[(size_t)k][(size_t)p] > 0 && (bk < 0 || cnt[(size_t)k][(size_t)p] > cnt[(size_t)bk][(size_t)bp])) { bk = k; bp = p; }
            if (bk < 0) break;
            ids[(size_t)bk] = (int32_t)bp; given[(size_t)bp] = 1;
        }
    }
    std::vector<int64_t> fk, fp;
    for (int64_t k = 0; k < K; ++k) if (ids[(size_t)k] < 0 && !nan_row(C + k * d)) fk.push_back(k);
    for (int64_t p = 0; p < P; ++p) if (!given[(size_t)p] && !nan_row(r.cen[(size_t)p].data())) fp.push_back(p);
    if (!fk.empty() && !fp.empty()) {
        std::vector<std::vector<double>> dist((size_t)K, std::vector<double>((size_t)P, NAN));
        for (int64_t k : fk) for (int64_t p : fp) {
            double dot = 0.0, m1 = 0.0, m2 = 0.0;
            for (int i = 0; i < d; ++i) { const double x = C[k * d + i], y = r.cen[(size_t)p][(size_t)i]; dot += x * y; m1 += x * x; m2 += y * y; }
            if (m1 == 0.0 || m2 == 0.0) return SD_ERR_NUMERIC;
            dist[(size_t)k][(size_t)p] = 1.0 - (dot / (sqrt(m1) * sqrt(m2)));
        }
        for (;;) {
            int64_t bk = -1, bp = -1;
            for (int64_t k : fk) for (int64_t p : fp)
                if (ids[(size_t)k] < 0 && !given[(size_t)p] && dist[(size_t)k][(size_t)p] <= t && (bk < 0 || dist[(size_t)k][(size_t)p] < dist[(size_t)bk][(size_t)bp])) { bk = k; bp = p; }
            if (bk < 0) break;
            ids[(size_t)bk] = (int32_t)bp; given[(size_t)bp] = 1;
        }
    }
    for (int64_t k = 0; k < K; ++k) if (ids[(size_t)k] < 0) { ids[(size_t)k] = (int32_t)r.n.size(); r.cen.emplace_back((size_t)d, 0.0); r.n.push_back(-1); r.seen.push_back(0); }
    for (int64_t k = 0; k < K; ++k) {
        const size_t p = (size_t)ids[(size_t)k];
        const int64_t mk = nan_row(C + k * d) ? 0 : m[k];
        if (r.n[p] < 0 || mk >= r.n[p]) { r.cen[p].assign(C + k * d, C + (k + 1) * d); r.n[p] = mk; }
        r.seen[p] = r.U;
    }
    r.U += 1;
    return SD_OK;
}

// ---- the roster's content, read through its public entries
struct Table { std::vector<double> cen; std::vector<int64_t> n, seen; int64_t P = 0, U = 0; int d = 0; };

static int read_table(const sd_roster* r, Table& t)
{
    CHECK(sd_roster_info(r, &t.P, &t.U, &t.d) == SD_OK, "info failed");
    t.cen.assign((size_t)(t.P * t.d), 0.0); t.n.assign((size_t)t.P, 0); t.seen.assign((size_t)t.P, 0);
    int64_t P2 = -1;
    CHECK(sd_roster_speakers(r, t.cen.data(), t.n.data(), t.seen.data(), t.P, &P2) == SD_OK && P2 == t.P, "speakers failed");
    return 0;
}
static bool same_table(const Table& a, const Table& b)
{
    return a.P == b.P && a.U == b.U && a.d == b.d && a.n == b.n && a.seen == b.seen &&
           (a.cen.empty() || memcmp(a.cen.data(), b.cen.data(), a.cen.size() * sizeof(double)) == 0);      // bytes: NaN rows included
}
static int against_naive(const sd_roster* r, const Naive& nv)
{
    Table t;
    if (read_table(r, t)) return 1;
    CHECK(t.P == (int64_t)nv.n.size() && t.U == nv.U && t.d == nv.d && t.n == nv.n && t.seen == nv.seen, "roster and naive table differ (P %lld / %zu, U %lld / %lld)",
          (long long)t.P, nv.n.size(), (long long)t.U, (long long)nv.U);
    for (int64_t p = 0; p < t.P; ++p) CHECK(memcmp(&t.cen[(size_t)(p * t.d)], nv.cen[(size_t)p].data(), (size_t)t.d * sizeof(double)) == 0, "centroid %lld differs", (long long)p);
    return 0;
}

// `call` with its first, second, ... allocation failing until it runs with none failing; every failure must be SD_ERR_NOMEM and change nothing
template <class F> static int every_allocation_failing(const sd_roster* r, F call, int* rc_out, long* failures)
{
    Table before;
    if (read_table(r, before)) return 1;
    for (long q = 0; ; ++q) {
        CHECK(q < 64, "a call with more than 64 allocations");
        g_fail_in = q;
        const int rc = call();
        const bool fired = g_fail_in == -1;
        g_fail_in = -1;
        if (!fired) { *rc_out = rc; return 0; }
        Table after;
        if (read_table(r, after)) return 1;
        CHECK(rc == SD_ERR_NOMEM && same_table(before, after), "allocation %ld failing: rc %d, roster %s", q, rc, same_table(before, after) ? "unchanged" : "CHANGED");
        ++*failures;
    }
}

struct Counts { long updates = 0, failures = 0, refusals = 0, numeric = 0, ties = 0, returns = 0; };

static int run_case(std::mt19937_64& rng, int steps, bool load, Counts& cs)
{
    const int d = 2 + (int)(rng() % 7);
    sd_roster* r = nullptr;
    int rc = 0;
    for (long q = 0; q < 2; ++q) {      // open: one allocation
        g_fail_in = q;
        rc = sd_roster_open(d, &r);
        const bool fired = g_fail_in == -1;
        g_fail_in = -1;
        if (!fired) break;
        CHECK(rc == SD_ERR_NOMEM && r == nullptr, "open with a failing allocation");
        ++cs.failures;
    }
    CHECK(rc == SD_OK && r, "open failed");
    Naive nv; nv.d = d;
    auto vec = [&](double* x) { for (int i = 0; i < d; ++i) x[i] = (double)((int)(rng() % 7) - 3); if (x[0] == 0.0 && rng() % 8) x[0] = 1.0; };      // a small grid: exact ties, now and then a zero row
    if (load) {
        const int64_t P = 1 + (int64_t)(rng() % 5);
        std::vector<double> cen((size_t)(P * d)); std::vector<int64_t> cnt((size_t)P);
        for (int64_t p = 0; p < P; ++p) { vec(&cen[(size_t)(p * d)]); cnt[(size_t)p] = (int64_t)(rng() % 20); }
        if (every_allocation_failing(r, [&]() { return sd_roster_load(r, cen.data(), cnt.data(), P); }, &rc, &cs.failures)) return 1;
        CHECK(rc == SD_OK, "load failed");
        for (int64_t p = 0; p < P; ++p) { nv.cen.emplace_back(cen.begin() + p * d, cen.begin() + (p + 1) * d); nv.n.push_back(cnt[(size_t)p]); nv.seen.push_back(-1); }
        CHECK(sd_roster_load(r, cen.data(), cnt.data(), P) == SD_ERR_ARG, "a second load was taken");
        if (against_naive(r, nv)) return 1;
    }
    std::vector<int32_t> kept;      // ids[rows[i]] of the previous update
    for (int step = 0; step < steps; ++step) {
        const int64_t K = (int64_t)(rng() % 7), M = (int64_t)(rng() % 61), P = (int64_t)nv.n.size();
        std::vector<double> C((size_t)(K * d) + 1); std::vector<int64_t> m((size_t)K + 1);
        for (int64_t k = 0; k < K; ++k) {
            vec(&C[(size_t)(k * d)]);
            m[(size_t)k] = (int64_t)(rng() % 30);
            const uint64_t how = rng() % 10;
            if (how == 0) C[(size_t)(k * d)] = NAN;
            if (how == 3 && rng() % 6 == 0) for (int i = 0; i < d; ++i) C[(size_t)(k * d + i)] = 0.0;      // a zero norm: SD_ERR_NUMERIC where step B reads it
            if (how == 1 && P > 0) { const size_t p = (size_t)(rng() % (uint64_t)P); memcpy(&C[(size_t)(k * d)], nv.cen[p].data(), (size_t)d * sizeof(double)); m[(size_t)k] = nv.n[p]; ++cs.ties; }      // an entry's own centroid and count
            if (how == 2 && k > 0) memcpy(&C[(size_t)(k * d)], &C[(size_t)((k - 1) * d)], (size_t)d * sizeof(double));      // two columns at equal distance from everything
        }
        std::vector<int32_t> rows((size_t)M + 1);
        for (int64_t i = 0; i < M; ++i) rows[(size_t)i] = K > 0 && rng() % 5 ? (int32_t)(rng() % (uint64_t)K) : -1 - (int32_t)(rng() % 2);
        const bool with_rows = rng() % 4 != 0, with_prev = !kept.empty() && rng() % 5 != 0;
        const int64_t shift = rng() % 3 ? 0 : (int64_t)(rng() % (uint64_t)(kept.size() + 4));      // now and then past the end of the previous table
        const double t = rng() % 6 == 0 ? NAN : rng() % 6 == 0 ? 0.0 : rng() % 6 == 0 ? 2.0 : 0.05 * (double)(rng() % 30);
        const int32_t* prows = with_rows ? rows.data() : nullptr;
        const int32_t* pprev = with_prev ? kept.data() : nullptr;
        const int64_t Mp = with_prev ? (int64_t)kept.size() : 0;
        std::vector<int32_t> ids((size_t)K + 1, -7), want;

        // the refusals, each leaving the roster what it was
        Table before, after;
        if (read_table(r, before)) return 1;
        CHECK(sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, -1, t, ids.data()) == SD_ERR_ARG, "a negative shift was taken");
        CHECK(sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, shift, 2.5, ids.data()) == SD_ERR_ARG, "a threshold of 2.5 was taken");
        if (K > 0) {
            CHECK(sd_roster_update(r, nullptr, m.data(), K, prows, M, pprev, Mp, shift, t, ids.data()) == SD_ERR_ARG, "null centroids were taken");
            CHECK(sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, shift, t, nullptr) == SD_ERR_ARG, "a null id array was taken");
            m[0] = -m[0] - 1;
            CHECK(sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, shift, t, ids.data()) == SD_ERR_ARG, "a negative count was taken");
            m[0] = -m[0] - 1;
        }
        if (with_rows && M > 0) {
            const int32_t was = rows[0];
            rows[0] = (int32_t)K;
            CHECK(sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, shift, t, ids.data()) == SD_ERR_ARG, "a row label of K was taken");
            rows[0] = was;
        }
        if (with_prev) {
            const int32_t was = kept[0];
            kept[0] = (int32_t)P;
            CHECK(sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, shift, t, ids.data()) == SD_ERR_ARG, "a previous id of P was taken");
            kept[0] = was;
        }
        cs.refusals += 2;
        if (read_table(r, after)) return 1;
        CHECK(same_table(before, after), "a refused update changed the roster");

        // the update, first with every allocation of it failing in turn
        Naive trial = nv;
        const int rc_want = naive_update(trial, C.data(), m.data(), K, prows, M, pprev, Mp, shift, t != t ? (double)0.7153814381597874f * (double)0.7153814381597874f / 2 : t, want);
        if (every_allocation_failing(r, [&]() { return sd_roster_update(r, C.data(), m.data(), K, prows, M, pprev, Mp, shift, t, ids.data()); }, &rc, &cs.failures)) return 1;
        CHECK(rc == rc_want, "step %d: rc %d, the naive rule gives %d", step, rc, rc_want);
        if (rc == SD_ERR_NUMERIC) {
            ++cs.numeric;
            if (read_table(r, after)) return 1;
            CHECK(same_table(before, after), "a zero-norm centroid changed the roster");
            continue;
        }
        nv = trial;
        for (int64_t k = 0; k < K; ++k) CHECK(ids[(size_t)k] == want[(size_t)k], "step %d: id of column %lld is %d, the naive rule gives %d", step, (long long)k, ids[(size_t)k], want[(size_t)k]);
        CHECK(ids[(size_t)K] == -7, "the id array was written past K");
        if (against_naive(r, nv)) return 1;
        for (int64_t k = 0; k < K; ++k) if (ids[(size_t)k] < P && before.seen[(size_t)ids[(size_t)k]] >= 0 && before.seen[(size_t)ids[(size_t)k]] < before.U - 1) ++cs.returns;
        ++cs.updates;
        if (with_rows) { kept.assign((size_t)M, -1); for (int64_t i = 0; i < M; ++i) if (rows[(size_t)i] >= 0) kept[(size_t)i] = ids[(size_t)rows[(size_t)i]]; }

        // the turns of this job under the map; a label outside it changes nothing
        std::vector<sd_turn> tv((size_t)K + 1);
        for (int64_t k = 0; k <= K; ++k) tv[(size_t)k] = sd_turn{(double)k, (double)k + 1.0, (int32_t)(K - k), 0};
        CHECK(sd_relabel_turns_map(tv.data(), K + 1, ids.data(), K) == SD_ERR_ARG && tv[0].label == (int32_t)K && (K == 0 || tv[1].label == (int32_t)(K - 1)), "a label of K was mapped");
        CHECK(sd_relabel_turns_map(tv.data() + 1, K, ids.data(), K) == SD_OK, "relabel failed");
        for (int64_t k = 1; k <= K; ++k) CHECK(tv[(size_t)k].label == ids[(size_t)(K - k)] && tv[(size_t)k].start == (double)k, "relabelled turn %lld", (long long)k);

        // the copy a group call takes, and putting it back
        if (rng() % 4 == 0) {
            sd_roster* copy = nullptr;
            if (every_allocation_failing(r, [&]() { return roster_copy(r, &copy); }, &rc, &cs.failures)) return 1;
            CHECK(rc == SD_OK && copy, "copy failed");
            Table tc;
            if (read_table(copy, tc) || read_table(r, before)) return 1;
            CHECK(same_table(tc, before), "the copy differs");
            double one[8] = {1, 1, 1, 1, 1, 1, 1, 1}; int64_t cnt1 = 1; int32_t id1 = -1;
            const int rc1 = sd_roster_update(r, one, &cnt1, 1, nullptr, 0, nullptr, 0, 0, 0.0, &id1);
            CHECK(rc1 == SD_OK || rc1 == SD_ERR_NUMERIC, "update behind the copy failed");      // (an entry made from a zero row that step B never had to read)
            roster_swap_tables(r, copy);
            if (read_table(r, after)) return 1;
            CHECK(same_table(before, after), "putting the copy back changed the roster");
            roster_free(copy);
        }
    }
    r->attached = 1;
    CHECK(sd_roster_close(r) == SD_ERR_ARG, "a roster with a stream attached was closed");
    r->attached = 0;
    CHECK(sd_roster_close(r) == SD_OK, "close failed");
    return 0;
}

int main(int argc, char** argv)
{
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 20241019ull);
    roster_alloc_hook = test_alloc;
    Counts cs;
    CHECK(sd_roster_open(0, nullptr) == SD_ERR_ARG && sd_roster_close(nullptr) == SD_OK && sd_roster_info(nullptr, nullptr, nullptr, nullptr) == SD_ERR_ARG &&
          sd_roster_speakers(nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SD_ERR_ARG && sd_roster_load(nullptr, nullptr, nullptr, 0) == SD_ERR_ARG &&
          sd_roster_update(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0, 0.5, nullptr) == SD_ERR_ARG && sd_relabel_turns_map(nullptr, 1, nullptr, 1) == SD_ERR_ARG,
          "a null pointer was taken");
    for (int q = 0; q < 120; ++q) if (run_case(rng, 12 + q % 20, q % 3 == 0, cs)) return 1;
    if (cs.updates < 1000 || cs.failures < 1000 || cs.numeric < 5 || cs.ties < 50 || cs.returns < 20) {
        printf("too little happened: %ld updates, %ld failed allocations, %ld zero norms, %ld ties, %ld returns\n", cs.updates, cs.failures, cs.numeric, cs.ties, cs.returns);
        return 1;
    }
    printf("roster ok: %ld updates, %ld failed allocations, %ld refusals, %ld zero norms, %ld returns, %ld allocations\n", cs.updates, cs.failures, cs.refusals, cs.numeric, cs.returns, g_allocs);
    return 0;
}
