#!/bin/bash
# CPU-only sanitizer build of the host bookkeeping of a stream with an input rate (csrc/resample_book.h: the rule F(n), the inputs kept, the rows of
# k_resample_jobs) with the device operations stubbed by malloc'd memory and the kernel body restated on the host: AddressSanitizer + UBSan.  Never
# loaded into python, never run on a GPU.
#   tools/sanitize/build_resample_book.sh <out-binary>;   <out-binary> [seed]   -> "resample_book ok" and exit 0; sanitizer reports go to stderr
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/resample_book_main.cpp -o "$1"
