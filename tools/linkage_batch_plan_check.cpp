// linkage_batch_plan_check.cpp -- the planner of run_linkage_many (csrc/linkage_batch_plan.h) as a program of its own, for a build with
// -fsanitize=address,undefined (tests/test_linkage_many_plan_cpu.py compiles and runs it; no GPU, no libsdhip.so).
//   every line of stdin = "<linkage_wgs> <linkage_one_xcd> <num_cu> <budget bytes> | <N_0> <N_1> ..."
//   prints "<single jobs> | <group> / <group> / ... | <bytes of job 0> <bytes of job 1> ..." per line (job numbers; the jobs of a group in launch order)
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
        long long wgs, onex, cu, budget;
        char bar = 0;
        if (!(in >> wgs >> onex >> cu >> budget >> bar) || bar != '|') { printf("bad line\n"); continue; }
        std::vector<int64_t> N;
        for (long long v; in >> v;) N.push_back(v);
        LinkageBatchPlan p;
        linkage_batch_plan(N.data(), (int64_t)N.size(), LinkageRoute{wgs, onex, (int)cu}, budget, p);
        for (int64_t j : p.single) printf("%lld ", (long long)j);
        printf("|");
        int64_t first = 0;
        for (size_t g = 0; g < p.group_end.size(); ++g) {
            if (g) printf(" /");
            for (int64_t k = first; k < p.group_end[g]; ++k) printf(" %lld", (long long)p.order[(size_t)k]);
            first = p.group_end[g];
        }
        printf(" |");
        for (int64_t n : N) printf(" %lld", (long long)(n >= 2 ? linkage_job_bytes(n) : 0));
        printf("\n");
    }
    return 0;
}
