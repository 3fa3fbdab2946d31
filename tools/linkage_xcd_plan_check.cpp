// linkage_xcd_plan_check.cpp -- the planner of the jobs run_linkage_many runs one per XCD (csrc/linkage_batch_plan.h: linkage_geometry, linkage_job_xcd,
// linkage_xcd_plan) as a program of its own, for a build with -fsanitize=address,undefined (tests/test_linkage_xcd_plan_cpu.py compiles and runs it; no GPU,
// no libsdhip.so).  It plans a call the way run_linkage_many does: linkage_batch_plan first, linkage_xcd_plan over the jobs that one left single.
//   every line of stdin = "<linkage_batch_xcd> <linkage_wgs> <linkage_one_xcd> <linkage_threads> <linkage_square> <linkage_kernel> <linkage_prefetch> <num_cu>
//                          <method> <linkage_force_heap> <budget bytes> | <N_0> <N_1> ..."
//   prints, per line, "<jobs of the one-workgroup batch> | <single jobs> | <group> / <group> ... | <job: eligible G TH helper cap bytes> , ..."
//   (job numbers; a group is its launches, separated by ";", the jobs of a launch in launch order)
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
        long long on, wgs, onex, threads, square, kernel, prefetch, cu, method, force, budget;
        char bar = 0;
        if (!(in >> on >> wgs >> onex >> threads >> square >> kernel >> prefetch >> cu >> method >> force >> budget >> bar) || bar != '|') { printf("bad line\n"); continue; }
        std::vector<int64_t> N;
        for (long long v; in >> v;) N.push_back(v);
        const LinkageXcdOpts x = {on, LinkageOpts{wgs, onex, threads, square, kernel, prefetch, (int)cu}, (int)method, force != 0, budget};
        LinkageBatchPlan p;
        linkage_batch_plan(N.data(), (int64_t)N.size(), LinkageRoute{wgs, onex, (int)cu}, budget, p);
        LinkageXcdPlan xp;
        linkage_xcd_plan(N.data(), p.single, x, xp);
        for (int64_t j : p.order) printf("%lld ", (long long)j);
        printf("| ");
        for (int64_t j : xp.single) printf("%lld ", (long long)j);
        printf("|");
        // both lists of ends rise strictly to the number of jobs, and a group's end is a launch's end: no launch lies in two groups
        const int64_t n = (int64_t)xp.order.size();
        bool ends = xp.key.size() == xp.order.size() && xp.group_end.empty() == (n == 0) && xp.launch_end.empty() == (n == 0);
        for (const std::vector<int64_t>* v : {&xp.group_end, &xp.launch_end})
            for (size_t i = 0; i < v->size(); ++i) ends = ends && (*v)[i] > (i ? (*v)[i - 1] : 0) && (*v)[i] <= n && (i + 1 < v->size() || (*v)[i] == n);
        for (int64_t e : xp.group_end) ends = ends && std::find(xp.launch_end.begin(), xp.launch_end.end(), e) != xp.launch_end.end();
        if (!ends) { printf(" BAD ENDS\n"); continue; }
        for (int64_t k = 0; k < n; ++k) {
            if (k > 0 && std::find(xp.group_end.begin(), xp.group_end.end(), k) != xp.group_end.end()) printf(" /");
            else if (k > 0 && std::find(xp.launch_end.begin(), xp.launch_end.end(), k) != xp.launch_end.end()) printf(" ;");
            printf(" %lld", (long long)xp.order[(size_t)k]);
        }
        printf(" |");
        for (size_t j = 0; j < N.size(); ++j) {
            LinkageXcdKey key = {0, 0, 0};
            const bool ok = linkage_job_xcd(x, N[j], &key);
            const LinkageGeom geo = linkage_geometry(x.o, N[j], true);
            printf("%s %d %d %d %d %d %lld", j ? " ," : "", ok ? 1 : 0, key.G, key.TH, key.helper, geo.G > 1 ? geo.cap : 0, (long long)(ok ? linkage_xcd_bytes(N[j], key.G) : 0));
        }
        printf("\n");
    }
    return 0;
}
