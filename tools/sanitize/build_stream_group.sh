#!/bin/bash
# CPU-only sanitizer build of the host planning of the group calls of sd_stream (csrc/stream_book.h: ranges to slots, the side of a range, growth
# before launch, the planned compaction) with the device operations stubbed by malloc'd memory: AddressSanitizer + UBSan.  Never loaded into
# python, never run on a GPU.
#   tools/sanitize/build_stream_group.sh <out-binary>;   <out-binary> run [seed] -> "stream_group ok" and exit 0;   <out-binary> plan <cases-file>;   <out-binary> tile <cases-file>
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/stream_group_main.cpp -o "$1"
