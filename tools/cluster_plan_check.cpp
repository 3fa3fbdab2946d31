// cluster_plan_check.cpp -- the host arithmetic of one cut of a dendrogram (csrc/cluster_host.h: cluster_plan) as a program of its own, for a build with
// -fsanitize=address,undefined (tests/test_cluster_plan_cpu.py compiles and runs it; no GPU, no libsdhip.so).
// stdin, per case: "N threshold min_cluster_size num_clusters min_clusters max_clusters" (-1 = unset), then the 4 (N - 1) numbers of Z
// stdout, per case: "<trivial> <mcs> <nl> | <labels> | <large> | <small> | <labels of the first cut>"
#include <cstdio>
#include <iostream>
#include "../pyannote-audio_speaker-diarization_cpp_amd/csrc/cluster_host.h"

static void print_list(const std::vector<int>& v)
{
    printf(" |");
    for (int x : v) printf(" %d", x);
}

int main()
{
    long long N;
    ClusterSpec s;
    while (std::cin >> N >> s.threshold >> s.min_cluster_size >> s.num_clusters >> s.min_clusters >> s.max_clusters) {
        if (N < 0) { fprintf(stderr, "bad N\n"); return 2; }
        std::vector<double> Z(N > 1 ? (size_t)(N - 1) * 4 : 0);
        for (double& z : Z) if (!(std::cin >> z)) { fprintf(stderr, "short Z\n"); return 2; }
        ClusterPlan p;
        std::vector<int> first;
        cluster_plan(Z, (int64_t)N, s, p, &first);
        printf("%d %zu %d", p.trivial ? 1 : 0, p.mcs, p.nl);
        print_list(p.lab); print_list(p.large); print_list(p.small); print_list(first);
        printf("\n");
    }
    return std::cin.eof() ? 0 : 2;
}
