// many_plan_check.cpp -- the host side of sd_diarize_many* (csrc/many_plan.h: the packed layout, the --many list reader) as a program of its own, for a
// build with -fsanitize=address,undefined (tests/test_many_plan.py compiles and runs it; no GPU, no libsdhip.so):
//   many_plan_check plan         every line of stdin = the lengths of one pack; prints "<base_0> .. <base_R-1> | <total>" or "refused" per line
//   many_plan_check list FILE    prints "ok <paths>" and one path per line, or "error: <message>"
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include "../pyannote-audio_speaker-diarization_cpp_amd/csrc/many_plan.h"

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "plan") == 0) {
        std::string line;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            std::vector<int64_t> n;
            for (long long v; in >> v;) n.push_back(v);
            std::vector<int64_t> base(n.size());
            int64_t total = -1;
            if (many_plan(n.empty() ? nullptr : n.data(), (int64_t)n.size(), base.data(), &total)) { printf("refused\n"); continue; }
            for (int64_t b : base) printf("%lld ", (long long)b);
            printf("| %lld\n", (long long)total);
        }
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "list") == 0) {
        std::vector<std::string> paths; std::string err;
        if (!many_read_list(argv[2], paths, err)) { printf("error: %s\n", err.c_str()); return 0; }
        printf("ok %zu\n", paths.size());
        for (const std::string& p : paths) printf("%s\n", p.c_str());
        return 0;
    }
    fprintf(stderr, "usage: many_plan_check plan < lists | many_plan_check list FILE\n");
    return 2;
}
