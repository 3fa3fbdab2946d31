// roster.cpp -- the speaker roster (roster.h; the rule is stated in sdhip.h under sd_roster_update and restated in tests/roster_ref.py).  Host only.
// An update computes everything into scratch memory first -- the ids of steps A, B and C, the grown table where new entries need room -- and changes
// the roster in a tail that cannot fail: a bad argument, a zero-norm centroid or a failed allocation leaves it exactly as it was.  The sums of the
// cosine distance are sequential f64 sums that must not be contracted into fused multiply-adds (sd.cpp:476-498; the bits of k_speaker_dist).
#include "roster.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#pragma STDC FP_CONTRACT OFF

void* (*roster_alloc_hook)(size_t bytes) = malloc;

namespace {
const double kDefaultThreshold = (double)0.7153814381597874f * (double)0.7153814381597874f / 2;      // option "speaker_match_threshold" as a context starts with it
const int64_t kMaxPairs = (int64_t)1 << 36;

void* ralloc(size_t bytes) { return roster_alloc_hook(bytes ? bytes : 1); }

struct RowPair { int64_t cnt; int32_t k, p; };
struct DistPair { double v; int32_t k, p; };

inline bool is_nan_row(const double* row) { return row[0] != row[0]; }

// room for `cap` entries in three fresh arrays holding the first r->P entries of r; false (nothing allocated) when an allocation fails
bool grown_tables(const sd_roster* r, int64_t cap, double** cen, int64_t** n, int64_t** seen)
{
    *cen = (double*)ralloc((size_t)cap * (size_t)r->d * sizeof(double));
    *n = *cen ? (int64_t*)ralloc((size_t)cap * sizeof(int64_t)) : nullptr;
    *seen = *n ? (int64_t*)ralloc((size_t)cap * sizeof(int64_t)) : nullptr;
    if (!*seen) { free(*cen); free(*n); *cen = nullptr; *n = nullptr; return false; }
    if (r->P > 0) {
        memcpy(*cen, r->cen, (size_t)r->P * (size_t)r->d * sizeof(double));
        memcpy(*n, r->n, (size_t)r->P * sizeof(int64_t));
        memcpy(*seen, r->seen, (size_t)r->P * sizeof(int64_t));
    }
    return true;
}
}

int roster_copy(const sd_roster* r, sd_roster** out)
{
    sd_roster* q = (sd_roster*)ralloc(sizeof(sd_roster));
    if (!q) return SD_ERR_NOMEM;
    *q = *r;
    q->attached = 0;
    q->cap = r->P > 0 ? r->P : 1;
    if (!grown_tables(r, q->cap, &q->cen, &q->n, &q->seen)) { free(q); return SD_ERR_NOMEM; }
    *out = q;
    return SD_OK;
}

void roster_swap_tables(sd_roster* a, sd_roster* b)
{
    std::swap(a->P, b->P); std::swap(a->cap, b->cap); std::swap(a->cen, b->cen); std::swap(a->n, b->n); std::swap(a->seen, b->seen);
    std::swap(a->updates, b->updates);
}

void roster_free(sd_roster* r)
{
    if (!r) return;
    free(r->cen); free(r->n); free(r->seen); free(r);
}

extern "C" int sd_roster_open(int d, sd_roster** out)
{
    if (!out || d < 1) return SD_ERR_ARG;
    sd_roster* r = (sd_roster*)ralloc(sizeof(sd_roster));
    if (!r) return SD_ERR_NOMEM;
    r->d = d; r->P = 0; r->cap = 0; r->cen = nullptr; r->n = nullptr; r->seen = nullptr; r->updates = 0; r->attached = 0;
    *out = r;
    return SD_OK;
}

extern "C" int sd_roster_close(sd_roster* r)
{
    if (!r) return SD_OK;
    if (r->attached > 0) return SD_ERR_ARG;      // a stream still holds it: detach (sd_stream_set_roster(s, NULL)) or close the stream first
    roster_free(r);
    return SD_OK;
}

extern "C" int sd_roster_load(sd_roster* r, const double* h_cen, const int64_t* h_counts, int64_t P)
{
    if (!r || P < 0 || P > 0x7fffffff || (P > 0 && (!h_cen || !h_counts)) || r->P != 0) return SD_ERR_ARG;
    for (int64_t p = 0; p < P; ++p) if (h_counts[p] < 0) return SD_ERR_ARG;
    if (P == 0) return SD_OK;
    sd_roster src = *r;      // (P = 0: grown_tables copies nothing)
    double* cen; int64_t* n; int64_t* seen;
    if (!grown_tables(&src, P, &cen, &n, &seen)) return SD_ERR_NOMEM;
    memcpy(cen, h_cen, (size_t)P * (size_t)r->d * sizeof(double));
    for (int64_t p = 0; p < P; ++p) { n[p] = is_nan_row(cen + p * r->d) ? 0 : h_counts[p]; seen[p] = -1; }
    free(r->cen); free(r->n); free(r->seen);
    r->cen = cen; r->n = n; r->seen = seen; r->P = P; r->cap = P;
    return SD_OK;
}

extern "C" int sd_roster_info(const sd_roster* r, int64_t* P, int64_t* updates, int* d)
{
    if (!r) return SD_ERR_ARG;
    if (P) *P = r->P;
    if (updates) *updates = r->updates;
    if (d) *d = r->d;
    return SD_OK;
}

extern "C" int sd_roster_speakers(const sd_roster* r, double* h_cen, int64_t* h_counts, int64_t* h_seen, int64_t cap, int64_t* P)
{
    if (!r || cap < 0) return SD_ERR_ARG;
    if (P) *P = r->P;
    const int64_t rows = cap < r->P ? cap : r->P;
    if (rows > 0) {
        if (h_cen) memcpy(h_cen, r->cen, (size_t)rows * (size_t)r->d * sizeof(double));
        if (h_counts) memcpy(h_counts, r->n, (size_t)rows * sizeof(int64_t));
        if (h_seen) memcpy(h_seen, r->seen, (size_t)rows * sizeof(int64_t));
    }
    return SD_OK;
}

extern "C" int sd_roster_update(sd_roster* r, const double* h_cen, const int64_t* h_counts, int64_t K, const int32_t* h_rows, int64_t M,
                                const int32_t* h_prev, int64_t Mp, int64_t shift, double threshold, int32_t* h_ids)
{
    // refusals: nothing is touched
    if (!r || K < 0 || (K > 0 && (!h_cen || !h_counts || !h_ids)) || M < 0 || Mp < 0 || shift < 0) return SD_ERR_ARG;
    if (threshold != threshold) threshold = kDefaultThreshold;
    else if (!(threshold >= 0.0 && threshold <= 2.0)) return SD_ERR_ARG;
    const int d = r->d;
    const int64_t P = r->P;
    if (K > 0x7fffffff - P) return SD_ERR_ARG;      // ids are int32
    for (int64_t k = 0; k < K; ++k) if (h_counts[k] < 0) return SD_ERR_ARG;
    if (h_rows) for (int64_t i = 0; i < M; ++i) if (h_rows[i] >= K) return SD_ERR_ARG;
    if (h_prev) for (int64_t j = 0; j < Mp; ++j) if (h_prev[j] >= P) return SD_ERR_ARG;
    int64_t n_over = 0;                              // rows this job shares with the previous one: i and i + shift
    if (h_rows && h_prev && shift < Mp) n_over = M < Mp - shift ? M : Mp - shift;

    // scratch, widest alignment first: codes [n_over] i64 | rp [n_over] RowPair | m1 [K] f64 | m2 [P] f64 | ids [K] | fk [K] | fp [P] i32 | given [P] char
    const size_t b_codes = (size_t)n_over * sizeof(int64_t), b_rp = (size_t)n_over * sizeof(RowPair), b_m1 = (size_t)K * sizeof(double),
                 b_m2 = (size_t)P * sizeof(double), b_k = (size_t)K * sizeof(int32_t), b_p = (size_t)P * sizeof(int32_t);
    char* scratch = (char*)ralloc(b_codes + b_rp + b_m1 + b_m2 + 2 * b_k + b_p + (size_t)P);
    if (!scratch) return SD_ERR_NOMEM;
    int64_t* codes = (int64_t*)scratch;
    RowPair* rp = (RowPair*)(scratch + b_codes);
    double* m1 = (double*)(scratch + b_codes + b_rp);
    double* m2 = (double*)(scratch + b_codes + b_rp + b_m1);
    int32_t* ids = (int32_t*)(scratch + b_codes + b_rp + b_m1 + b_m2);
    int32_t* fk = ids + K;
    int32_t* fp = fk + K;
    char* given = (char*)(fp + P);
    for (int64_t k = 0; k < K; ++k) ids[k] = -1;
    if (P > 0) memset(given, 0, (size_t)P);

    // A, rows: cnt[k][p] over the shared rows, pairs in (-cnt, k, p) order, a pair taken when both sides are free
    int64_t nq = 0;
    for (int64_t i = 0; i < n_over; ++i) {
        const int32_t k = h_rows[i], p = h_prev[i + shift];
        if (k >= 0 && p >= 0) codes[nq++] = (int64_t)k * P + p;
    }
    std::sort(codes, codes + nq);
    int64_t np = 0;
    for (int64_t q = 0; q < nq; ) {
        int64_t e = q;
        while (e < nq && codes[e] == codes[q]) ++e;
        rp[np++] = RowPair{e - q, (int32_t)(codes[q] / P), (int32_t)(codes[q] % P)};
        q = e;
    }
    std::sort(rp, rp + np, [](const RowPair& a, const RowPair& b) { return a.cnt != b.cnt ? a.cnt > b.cnt : a.k != b.k ? a.k < b.k : a.p < b.p; });
    for (int64_t q = 0; q < np; ++q)
        if (ids[rp[q].k] < 0 && !given[rp[q].p]) { ids[rp[q].k] = rp[q].p; given[rp[q].p] = 1; }

    // B, centroids: the rule of sd_match_speakers over the k that are still free and the entries this update has not given out
    int64_t nfk = 0, nfp = 0;
    for (int64_t k = 0; k < K; ++k) if (ids[k] < 0 && !is_nan_row(h_cen + k * d)) fk[nfk++] = (int32_t)k;
    for (int64_t p = 0; p < P; ++p) if (!given[p] && !is_nan_row(r->cen + p * d)) fp[nfp++] = (int32_t)p;
    if (nfk > 0 && nfp > 0) {
        bool zero = false;
        for (int64_t a = 0; a < nfk; ++a) {
            const double* x = h_cen + (int64_t)fk[a] * d;
            double s = 0.0;
            for (int i = 0; i < d; ++i) s += x[i] * x[i];
            m1[a] = s; zero |= s == 0.0;
        }
        for (int64_t b = 0; b < nfp; ++b) {
            const double* y = r->cen + (int64_t)fp[b] * d;
            double s = 0.0;
            for (int i = 0; i < d; ++i) s += y[i] * y[i];
            m2[b] = s; zero |= s == 0.0;
        }
        if (zero) { free(scratch); return SD_ERR_NUMERIC; }      // the reference throws, sd.cpp:493-495
        if (nfk > kMaxPairs / nfp) { free(scratch); return SD_ERR_NOMEM; }
        DistPair* dp = (DistPair*)ralloc((size_t)(nfk * nfp) * sizeof(DistPair));
        if (!dp) { free(scratch); return SD_ERR_NOMEM; }
        int64_t nd = 0;
        for (int64_t a = 0; a < nfk; ++a) {
            const double* x = h_cen + (int64_t)fk[a] * d;
            for (int64_t b = 0; b < nfp; ++b) {
                const double* y = r->cen + (int64_t)fp[b] * d;
                double dot = 0.0;
                for (int i = 0; i < d; ++i) dot += x[i] * y[i];
                const double v = 1.0 - (dot / (sqrt(m1[a]) * sqrt(m2[b])));
                if (v <= threshold) dp[nd++] = DistPair{v, fk[a], fp[b]};
            }
        }
        std::sort(dp, dp + nd, [](const DistPair& a, const DistPair& b) { return a.v != b.v ? a.v < b.v : a.k != b.k ? a.k < b.k : a.p < b.p; });
        for (int64_t q = 0; q < nd; ++q)
            if (ids[dp[q].k] < 0 && !given[dp[q].p]) { ids[dp[q].k] = dp[q].p; given[dp[q].p] = 1; }
        free(dp);
    }

    // C: new ids P, P + 1, ... in ascending k; the table grows before anything is committed
    int64_t fresh = 0;
    for (int64_t k = 0; k < K; ++k) if (ids[k] < 0) ids[k] = (int32_t)(P + fresh++);
    if (P + fresh > r->cap) {
        int64_t cap = r->cap * 2 > 8 ? r->cap * 2 : 8;
        if (cap < P + fresh) cap = P + fresh;
        double* cen; int64_t* n; int64_t* seen;
        if (!grown_tables(r, cap, &cen, &n, &seen)) { free(scratch); return SD_ERR_NOMEM; }
        free(r->cen); free(r->n); free(r->seen);
        r->cen = cen; r->n = n; r->seen = seen; r->cap = cap;      // the same P entries in larger arrays: the roster is still what it was
    }

    // D, refresh: nothing below can fail.  An entry keeps the estimate made from the most rows; a tie goes to the later one
    for (int64_t k = 0; k < K; ++k) {
        const int64_t p = ids[k];
        const int64_t mk = is_nan_row(h_cen + k * d) ? 0 : h_counts[k];
        if (p >= P || mk >= r->n[p]) { memcpy(r->cen + p * d, h_cen + k * d, (size_t)d * sizeof(double)); r->n[p] = mk; }
        r->seen[p] = r->updates;
        h_ids[k] = (int32_t)p;
    }
    r->P = P + fresh;
    r->updates += 1;
    free(scratch);
    return SD_OK;
}

extern "C" int sd_relabel_turns_map(sd_turn* turns, int64_t n_turns, const int32_t* ids, int64_t K)
{
    if (n_turns < 0 || K < 0 || (n_turns > 0 && (!turns || !ids))) return SD_ERR_ARG;
    for (int64_t i = 0; i < n_turns; ++i) if (turns[i].label < 0 || turns[i].label >= K) return SD_ERR_ARG;      // nothing is written
    for (int64_t i = 0; i < n_turns; ++i) turns[i].label = ids[turns[i].label];
    return SD_OK;
}
