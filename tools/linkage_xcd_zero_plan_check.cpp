// linkage_xcd_zero_plan_check.cpp -- which jobs of an XCD launch that tie at height 0 stay in the batch, and in which zero launches (csrc/linkage_batch_plan.h:
// linkage_tie_plan, linkage_hx_form, linkage_job_xcd_zero, linkage_xcd_zero_plan, linkage_xcd_zero_bytes; option "linkage_batch_xcd_zero") as a
// program of its own, for a build with -fsanitize=address,undefined (tests/test_linkage_xcd_zero_plan_cpu.py compiles and runs it; no GPU, no libsdhip.so).
//   every line of stdin = "<linkage_batch_xcd_zero> <linkage_zero_phase> <linkage_tie_kernel> <linkage_one_xcd> <linkage_hx_wide> <num_cu> |
//                          <N G TH helper ran timeout tie tie_bits untouched> , <...> ..."      (one record per job the first launches left unfinished, plan order)
//   prints, per line, "<launch> ; <launch> ... | <job: why workers replay hx_onex s16 lc dyn cap bytes> , ..."
//   (a launch is the numbers of its jobs in launch order; why = LinkageZeroWhy, 0 = in a launch)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../pyannote-audio_speaker-diarization_cpp_amd/csrc/linkage_batch_plan.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        long long on, zero_phase, tie_kernel, onex, wide, cu;
        char bar = 0;
        if (!(in >> on >> zero_phase >> tie_kernel >> onex >> wide >> cu >> bar) || bar != '|') { printf("bad line\n"); continue; }
        const LinkageXcdZeroOpts o = {on, zero_phase, tie_kernel, onex, wide != 0, (int)cu};
        std::vector<LinkageXcdZeroJob> jobs;
        bool bad = false;
        for (;;) {
            long long N, G, TH, helper, ran, timeout, tie, untouched;
            unsigned long long bits;
            if (!(in >> N)) break;
            if (!(in >> G >> TH >> helper >> ran >> timeout >> tie >> bits >> untouched)) { bad = true; break; }
            jobs.push_back(LinkageXcdZeroJob{N, LinkageXcdKey{(int)G, (int)TH, (int)helper}, ran != 0, timeout != 0, tie != 0, (uint64_t)bits, untouched != 0});
            char comma = 0;
            if (!(in >> comma)) break;
            if (comma != ',') { bad = true; break; }
        }
        if (bad) { printf("bad line\n"); continue; }
        LinkageXcdZeroPlan p;
        linkage_xcd_zero_plan(jobs.data(), (int64_t)jobs.size(), o, p);
        // the ends rise strictly to the size of the zero set; one worker count per job of it; one reason per job of the input
        const int64_t n = (int64_t)p.order.size();
        bool ends = p.workers.size() == p.order.size() && p.why.size() == jobs.size() && p.launch_end.empty() == (n == 0);
        for (size_t i = 0; i < p.launch_end.size(); ++i)
            ends = ends && p.launch_end[i] > (i ? p.launch_end[i - 1] : 0) && p.launch_end[i] <= n && (i + 1 < p.launch_end.size() || p.launch_end[i] == n);
        if (!ends) { printf("BAD ENDS\n"); continue; }
        for (int64_t k = 0; k < n; ++k) {
            if (k > 0 && std::find(p.launch_end.begin(), p.launch_end.end(), k) != p.launch_end.end()) printf(" ;");
            printf(" %lld", (long long)p.order[(size_t)k]);
        }
        printf(" |");
        for (size_t j = 0; j < jobs.size(); ++j) {
            int workers = 0;
            const LinkageZeroWhy why = linkage_job_xcd_zero(o, jobs[j], &workers);
            const LinkageTie t = linkage_tie_plan(tie_kernel, onex, (int)cu, jobs[j].N, true);
            bool s16; int lc; size_t dyn;
            linkage_hx_form(jobs[j].N, wide != 0, s16, lc, dyn);
            const bool same = why == p.why[j];
            printf("%s %d %d %d %d %d %d %lld %lld %lld%s", j ? " ," : "", (int)why, t.workers, t.replay ? 1 : 0, t.hx_onex ? 1 : 0, s16 ? 1 : 0, lc, (long long)dyn,
                   (long long)(why == ZERO_IN ? linkage_xcd_zero_cap(jobs[j].N, workers) : 0), (long long)(why == ZERO_IN ? linkage_xcd_zero_bytes(jobs[j].N, workers) : 0),
                   same ? "" : " BAD WHY");
        }
        printf("\n");
    }
    return 0;
}
