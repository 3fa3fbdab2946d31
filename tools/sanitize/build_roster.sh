#!/bin/bash
# CPU-only sanitizer build of the speaker roster (csrc/roster.cpp, the file the library is built from, next to a naive second implementation of its
# rule): AddressSanitizer + UBSan, no FMA contraction as in the library.  Never loaded into python, never run on a GPU.
#   tools/sanitize/build_roster.sh <out-binary>;   <out-binary> [seed] -> "roster ok" and exit 0
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/roster_main.cpp $src/roster.cpp -o "$1"
