// linkage_heap.hip -- k_linkage_heap: the reference's linkage (fast_linkage, cl.cpp:289-406) on ONE workgroup, its binary heap replayed operation by
// operation, on the condensed distance matrix; all seven methods.  run_linkage (linkage.hip) takes it for small N and as the last resort behind k_linkage_hx.
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"

// (the body, heap_linkage, with scan_row_nn, block_min and the heap operations hp_*, is linkage_dev.h's: k_linkage_heap_jobs calls the same function)
#define LT 1024

// ---------------------------------------------------------------- k_linkage_heap : persistent single workgroup, the reference's heap included
// The heap (values / key_by_index / index_by_key) lives in LDS up to HEAP_LDS entries, in global memory above.
#define HEAP_LDS 2048
static_assert(HEAP_LDS == LINKAGE_HEAP_LDS, "linkage_batch_plan.h batches the jobs whose heap fits this kernel's LDS heap");
template <int METHOD>
__global__ __launch_bounds__(LT) void k_linkage_heap(double* D, int n, int* size, int* cid, int* nb, double* md, double* Z,
                                                      double* g_hval, int* g_hkey, int* g_hpos)
{
    extern __shared__ unsigned changed[];                 // bitmap of the rows whose bound dropped in this merge
    __shared__ MinIdx sh[LT / 64];
    __shared__ HeapShared s;
    __shared__ double s_hv[HEAP_LDS];
    __shared__ int s_hk[HEAP_LDS], s_hp[HEAP_LDS];
    const bool in_lds = (n - 1) <= HEAP_LDS;
    HeapRef h;
    h.val = in_lds ? s_hv : g_hval; h.key = in_lds ? s_hk : g_hkey; h.pos = in_lds ? s_hp : g_hpos; h.size = n - 1;
    heap_linkage<METHOD, LT>(D, n, size, cid, nb, md, Z, h, changed, sh, s);
}

// launcher (declared in linkage_dev.h): Dc = condensed matrix, nb / md = exact nearest neighbours above each row, size = 1, cid = iota (LinkageJob::prepare)
int linkage_heap_run(sd_ctx* c, int method, double* Dc, int64_t N, int* size, int* cid, int* nb, double* md, double* d_Z)
{
    double* hval = nullptr; int* hkey = nullptr; int* hpos = nullptr;
    if (N - 1 > HEAP_LDS) {
        WS(c, double, hv, "cl_hval", N);
        WS(c, int, hk, "cl_hkey", N);
        WS(c, int, hp, "cl_hpos", N);
        hval = hv; hkey = hk; hpos = hp;
    }
    ProfScope ps(c, "linkage_heap", 0, 24.0 * (double)N * (double)N);
    const bool known = lw_dispatch(method, [&](auto M) {
        hipLaunchKernelGGL(k_linkage_heap<M.value>, dim3(1), dim3(LT), (size_t)((N + 31) / 32) * sizeof(unsigned), c->stream, Dc, (int)N, size, cid, nb, md, d_Z, hval, hkey, hpos); });
    if (!known) SD_FAIL(c, SD_ERR_ARG, "k_linkage_heap: no linkage method %d", method);
    KCHECK(c);
    return SD_OK;
}
