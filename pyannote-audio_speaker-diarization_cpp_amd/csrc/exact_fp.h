// exact_fp.h -- included by every file whose fp64 bits must equal the reference's x86 build: refuses a build without the Makefile's $(EXACT) flags
#ifndef SD_EXACT_FP
#error "this file needs exact fp64 arithmetic: compile it with -ffp-contract=off -DSD_EXACT_FP (Makefile: EXACT; list the file in SRC_EXACT)"
#endif
