#!/bin/bash
# CPU-only sanitizer build of the sliding window of sd_stream (csrc/stream_book.h: book_forget, next to the reserve / seal / group steps it follows)
# with the device operations stubbed by malloc'd memory: AddressSanitizer + UBSan.  Never loaded into python, never run on a GPU.
#   tools/sanitize/build_stream_window.sh <out-binary>;   <out-binary> [seed] -> "stream_window ok" and exit 0
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/stream_window_main.cpp -o "$1"
