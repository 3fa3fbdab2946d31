// der.cpp -- scoring against a ground truth, on the host alone: the diarization error rate of include/sdhip.h (sd_der; the rule of pyannote.metrics'
// DiarizationErrorRate, restated there) and the reader of the RTTM files sd_write_rttm* and pyannote write (sd_read_rttm).  No GPU work, no context.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "../../include/sdhip.h"

static std::string g_score_err;
extern "C" const char* sd_score_error(void) { return g_score_err.c_str(); }
static int score_fail(const std::string& m) { g_score_err = m; return SD_ERR_ARG; }

namespace {
// a sum of f64 terms that carries its rounding errors along (Neumaier): the result is the exact sum rounded once, to a part in 2^53 of the sums of this file
struct Acc {
    double s = 0.0, c = 0.0;
    void add(double x) { const double t = s + x; c += std::fabs(s) >= std::fabs(x) ? (s - t) + x : (x - t) + s; s = t; }
    void add_times(double x, int m) { for (int i = 0; i < m; ++i) add(x); }
    double value() const { return s + c; }
};

// Rectangular linear sum assignment, minimised: shortest augmenting paths with dual variables (Crouse, "On implementing 2D rectangular assignment
// algorithms", IEEE TAES 2016), any nr <= nc.  col4row[i] = the column of row i.
void lsap_min(int nr, int nc, const std::vector<double>& cost, std::vector<int>& col4row)
{
    std::vector<double> u((size_t)nr, 0.0), v((size_t)nc, 0.0), spc((size_t)nc);
    std::vector<int> path((size_t)nc, -1), row4col((size_t)nc, -1), remaining((size_t)nc);
    std::vector<char> SR((size_t)nr), SC((size_t)nc);
    col4row.assign((size_t)nr, -1);
    for (int cur = 0; cur < nr; ++cur) {
        double minVal = 0.0;
        int num_remaining = nc, sink = -1, i = cur;
        for (int it = 0; it < nc; ++it) remaining[(size_t)it] = nc - it - 1;
        std::fill(SR.begin(), SR.end(), 0);
        std::fill(SC.begin(), SC.end(), 0);
        std::fill(spc.begin(), spc.end(), INFINITY);
        while (sink == -1) {
            int index = -1; double lowest = INFINITY;
            SR[(size_t)i] = 1;
            for (int it = 0; it < num_remaining; ++it) {
                const int j = remaining[(size_t)it];
                const double r = minVal + cost[(size_t)i * nc + j] - u[(size_t)i] - v[(size_t)j];
                if (r < spc[(size_t)j]) { path[(size_t)j] = i; spc[(size_t)j] = r; }
                if (spc[(size_t)j] < lowest || (spc[(size_t)j] == lowest && row4col[(size_t)j] == -1)) { lowest = spc[(size_t)j]; index = it; }
            }
            minVal = lowest;
            if (index < 0) return;                                   // (finite costs: cannot happen)
            const int j = remaining[(size_t)index];
            if (row4col[(size_t)j] == -1) sink = j; else i = row4col[(size_t)j];
            SC[(size_t)j] = 1;
            remaining[(size_t)index] = remaining[(size_t)--num_remaining];
        }
        u[(size_t)cur] += minVal;
        for (int r = 0; r < nr; ++r) if (SR[(size_t)r] && r != cur) u[(size_t)r] += minVal - spc[(size_t)col4row[(size_t)r]];
        for (int j = 0; j < nc; ++j) if (SC[(size_t)j]) v[(size_t)j] -= minVal - spc[(size_t)j];
        for (int j = sink;;) {
            const int r = path[(size_t)j];
            row4col[(size_t)j] = r;
            std::swap(col4row[(size_t)r], j);
            if (r == cur) break;
        }
    }
}

// kind of a time-line event: a turn of the reference / of the hypothesis (idx = its dense label), a span of the uem, a collar zone
enum { EV_REF = 0, EV_HYP = 1, EV_UEM = 2, EV_COLLAR = 3 };
struct Event { double t; int kind, idx, delta; };

int check_turns(const sd_turn* t, int64_t n, const char* what, bool labels)
{
    if (n < 0 || (n > 0 && !t)) return score_fail(std::string("sd_der: bad argument (") + what + ")");
    for (int64_t i = 0; i < n; ++i) {
        if (!(t[i].start >= 0.0) || !(t[i].end >= t[i].start) || !std::isfinite(t[i].end))
            return score_fail(std::string("sd_der: ") + what + " " + std::to_string(i) + ": times must be numbers with 0 <= start <= end");
        if (labels && t[i].label < 0) return score_fail(std::string("sd_der: ") + what + " " + std::to_string(i) + " has a negative label");
    }
    return SD_OK;
}

std::vector<int32_t> dense_labels(const sd_turn* t, int64_t n, std::vector<int>& idx)
{
    std::vector<int32_t> u;
    for (int64_t i = 0; i < n; ++i) u.push_back(t[i].label);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    idx.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) idx[(size_t)i] = (int)(std::lower_bound(u.begin(), u.end(), t[i].label) - u.begin());
    return u;
}
}

extern "C" int sd_der(const sd_turn* ref, int64_t n_ref, const sd_turn* hyp, int64_t n_hyp, const sd_turn* uem, int64_t n_uem, double collar,
                      int skip_overlap, sd_der_result* result, int32_t* map, int64_t cap, int64_t* n_map)
{
    g_score_err.clear();
    if (!result || cap < 0 || (cap > 0 && !map)) return score_fail("sd_der: bad argument");
    if (!(collar >= 0.0) || !std::isfinite(collar)) return score_fail("sd_der: collar must be a number of seconds >= 0");
    if (int rc = check_turns(ref, n_ref, "reference turn", true)) return rc;
    if (int rc = check_turns(hyp, n_hyp, "hypothesis turn", true)) return rc;
    if (!uem) n_uem = 0;
    if (int rc = check_turns(uem, n_uem, "uem span", false)) return rc;

    std::vector<int> ri, hi;
    const std::vector<int32_t> rlab = dense_labels(ref, n_ref, ri), hlab = dense_labels(hyp, n_hyp, hi);
    const int R = (int)rlab.size(), H = (int)hlab.size();
    std::vector<Event> ev;
    ev.reserve((size_t)(4 * n_ref + 2 * n_hyp + 2 * n_uem));
    const double half = collar / 2;
    for (int64_t i = 0; i < n_ref; ++i) {
        ev.push_back({ref[i].start, EV_REF, ri[(size_t)i], 1}); ev.push_back({ref[i].end, EV_REF, ri[(size_t)i], -1});
        if (collar > 0.0)
            for (const double t : {ref[i].start, ref[i].end}) { ev.push_back({t - half, EV_COLLAR, 0, 1}); ev.push_back({t + half, EV_COLLAR, 0, -1}); }
    }
    for (int64_t i = 0; i < n_hyp; ++i) { ev.push_back({hyp[i].start, EV_HYP, hi[(size_t)i], 1}); ev.push_back({hyp[i].end, EV_HYP, hi[(size_t)i], -1}); }
    for (int64_t i = 0; i < n_uem; ++i) { ev.push_back({uem[i].start, EV_UEM, 0, 1}); ev.push_back({uem[i].end, EV_UEM, 0, -1}); }
    std::stable_sort(ev.begin(), ev.end(), [](const Event& a, const Event& b) { return a.t < b.t; });

    // one walk over the elementary intervals in ascending time: fn(D, A, B) for every scored one, A / B = the dense labels that are on
    auto walk = [&](auto&& fn) {
        std::vector<int> rc((size_t)R, 0), hc((size_t)H, 0), A, B;
        int in_uem = 0, in_collar = 0;
        for (size_t e = 0; e < ev.size();) {
            const double x0 = ev[e].t;
            for (; e < ev.size() && ev[e].t == x0; ++e) {
                const Event& q = ev[e];
                if (q.kind == EV_REF) rc[(size_t)q.idx] += q.delta; else if (q.kind == EV_HYP) hc[(size_t)q.idx] += q.delta;
                else if (q.kind == EV_UEM) in_uem += q.delta; else in_collar += q.delta;
            }
            if (e == ev.size()) break;
            if ((uem && !in_uem) || in_collar) continue;
            A.clear(); B.clear();
            for (int a = 0; a < R; ++a) if (rc[(size_t)a] > 0) A.push_back(a);
            for (int b = 0; b < H; ++b) if (hc[(size_t)b] > 0) B.push_back(b);
            if ((A.empty() && B.empty()) || (skip_overlap && A.size() >= 2)) continue;
            fn(ev[e].t - x0, A, B);
        }
    };

    // the mapping: the one-to-one pairing of reference and hypothesis labels with the largest summed co-occurrence
    std::vector<int> h4r((size_t)R, -1);
    if (R > 0 && H > 0) {
        std::vector<Acc> co((size_t)R * H);
        walk([&](double D, const std::vector<int>& A, const std::vector<int>& B) { for (int a : A) for (int b : B) co[(size_t)a * H + b].add(D); });
        const bool tr = R > H;                                        // the solver wants no more rows than columns
        const int nr = tr ? H : R, nc = tr ? R : H;
        std::vector<double> cost((size_t)nr * nc);
        for (int a = 0; a < R; ++a) for (int b = 0; b < H; ++b) cost[tr ? (size_t)b * nc + a : (size_t)a * nc + b] = -co[(size_t)a * H + b].value();
        std::vector<int> c4r;
        lsap_min(nr, nc, cost, c4r);
        for (int i = 0; i < nr; ++i) if (c4r[(size_t)i] >= 0) { if (tr) h4r[(size_t)c4r[(size_t)i]] = i; else h4r[(size_t)i] = c4r[(size_t)i]; }
        for (int a = 0; a < R; ++a) if (h4r[(size_t)a] >= 0 && !(co[(size_t)a * H + h4r[(size_t)a]].value() > 0.0)) h4r[(size_t)a] = -1;      // a pair that never meets is no pair
    }

    Acc total, missed, fa, correct, confusion;
    std::vector<char> on((size_t)H);
    walk([&](double D, const std::vector<int>& A, const std::vector<int>& B) {
        const int na = (int)A.size(), nb = (int)B.size();
        std::fill(on.begin(), on.end(), 0);
        for (int b : B) on[(size_t)b] = 1;
        int ok = 0;
        for (int a : A) if (h4r[(size_t)a] >= 0 && on[(size_t)h4r[(size_t)a]]) ++ok;
        total.add_times(D, na);
        missed.add_times(D, std::max(0, na - nb));
        fa.add_times(D, std::max(0, nb - na));
        correct.add_times(D, ok);
        confusion.add_times(D, std::min(na, nb) - ok);
    });
    result->total = total.value(); result->missed = missed.value(); result->false_alarm = fa.value();
    result->correct = correct.value(); result->confusion = confusion.value();
    result->der = result->total > 0.0 ? (result->missed + result->false_alarm + result->confusion) / result->total : NAN;

    const int64_t nm = H > 0 ? (int64_t)hlab.back() + 1 : 0;
    if (n_map) *n_map = nm;
    for (int64_t h = 0; h < nm && h < cap; ++h) map[h] = -1;
    for (int a = 0; a < R; ++a) if (h4r[(size_t)a] >= 0 && (int64_t)hlab[(size_t)h4r[(size_t)a]] < cap) map[hlab[(size_t)h4r[(size_t)a]]] = rlab[(size_t)a];
    return SD_OK;
}

// "SPEAKER <uri> <channel> <start> <duration> <NA> <NA> <name> ..." lines; other record types of the format and ;; comments are passed over
extern "C" int sd_read_rttm(const char* path, const char* uri, sd_turn** turns, int64_t* n, char*** names, int64_t* K)
{
    g_score_err.clear();
    if (!path || !turns || !n) return score_fail("sd_read_rttm: bad argument");
    *turns = nullptr; *n = 0;
    if (names) *names = nullptr;
    if (K) *K = 0;
    std::ifstream in(path);
    if (!in) return score_fail(std::string("cannot open ") + path);
    std::vector<sd_turn> v;
    std::vector<std::string> nm;
    std::string line;
    auto bad = [&](int64_t no, const std::string& why) { return score_fail(std::string(path) + ": line " + std::to_string(no) + ": " + why); };
    for (int64_t no = 1; std::getline(in, line); ++no) {
        std::vector<std::string> tok;
        for (size_t i = 0; i < line.size();) {
            while (i < line.size() && (line[i] == ' ' || (line[i] >= '\t' && line[i] <= '\r'))) ++i;
            size_t j = i;
            while (j < line.size() && !(line[j] == ' ' || (line[j] >= '\t' && line[j] <= '\r'))) ++j;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
        if (tok.empty() || tok[0].compare(0, 2, ";;") == 0 || tok[0] != "SPEAKER") continue;
        if (tok.size() < 8) return bad(no, "a SPEAKER line has at least 8 fields, " + std::to_string(tok.size()) + " found");
        double val[2];
        for (int q = 0; q < 2; ++q) {
            char* end = nullptr;
            val[q] = strtod(tok[(size_t)3 + q].c_str(), &end);
            if (end == tok[(size_t)3 + q].c_str() || *end || !std::isfinite(val[q]) || val[q] < 0.0)
                return bad(no, "'" + tok[(size_t)3 + q] + "' is not a " + (q ? "duration" : "start time") + " >= 0");
        }
        if (uri && tok[1] != uri) continue;
        size_t k = (size_t)(std::find(nm.begin(), nm.end(), tok[7]) - nm.begin());
        if (k == nm.size()) nm.push_back(tok[7]);
        v.push_back(sd_turn{val[0], val[0] + val[1], (int32_t)k, 0});
    }
    sd_turn* t = (sd_turn*)malloc(sizeof(sd_turn) * (v.size() ? v.size() : 1));
    char** pn = names ? (char**)malloc(sizeof(char*) * (nm.size() ? nm.size() : 1)) : nullptr;
    if (!t || (names && !pn)) { free(t); free(pn); return score_fail("out of host memory"); }
    for (size_t i = 0; i < v.size(); ++i) t[i] = v[i];
    if (names) { for (size_t i = 0; i < nm.size(); ++i) pn[i] = strdup(nm[i].c_str()); *names = pn; }
    *turns = t; *n = (int64_t)v.size();
    if (K) *K = (int64_t)nm.size();
    return SD_OK;
}

extern "C" void sd_free_rttm_names(char** names, int64_t K)
{
    if (names) for (int64_t i = 0; i < K; ++i) free(names[i]);
    free(names);
}
