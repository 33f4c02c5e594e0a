// Point-to-point messages that read or write a derived datatype in the kernel
// that moves them (include/ompi_amd_p2p.h's *_typed forms).
//
// The wire format is the packed stream, so each kernel has one typed end (the
// caller's buffer) and one contiguous end (library memory: an eager cell, a
// send stage, or whatever a byte sender published):
//   eager_put_typed   typed -> cell, then eager_put's publication;
//   eager_get_typed   eager_get's wait, then cell -> typed;
//   xfer_pack_sig     typed -> send stage, xfer_copy_sig's persistent grid and
//                     last-workgroup signal;
//   xfer_unpack_sig   every workgroup waits for the stage's flag, then
//                     stage -> typed; the stores are local, so the kernel
//                     boundary ends it.
// The walk is coll_kernels.h's typed_pipe_copy (granule and 32-/64-bit choice:
// coll_typed.h); the element program sits in LDS when it fits the alltoallw
// kernels' budget (kA2awLdsElems) and is walked from global memory otherwise.
//
// One kernel has a datatype on both ends and no contiguous end at all
// (DESIGN.md §3.8):
//   ddt_sndrcv        typed -> typed through coll_kernels.h's typed_pipe_copy2,
//                     both programs in the same LDS budget.  It is the local
//                     copy ompi_amd_ddt_sndrcv (include/ompi_amd_ddt.h) and the
//                     receiver's half of the typed rendezvous, where the source
//                     buffer and the source program are a peer's mapped memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../include/ompi_amd_p2p.h"
#include "coll_kernels.h"
#include "comm_internal.h"
#include "runtime.h"

namespace ompi_amd {

// The kernel's own copy of its typed end; with `lds` its program moves into
// `prog` first and the walk's element search reads LDS.
__device__ __forceinline__ typed_end staged_end(const typed_end &arg, ddt_elem *prog, int lds) {
    typed_end e = arg;
    if (lds) {
        lds_words(prog, arg.d.elems, arg.d.nelem * (int)(sizeof(ddt_elem) / sizeof(uint64_t)));
        __syncthreads();
        e.d.elems = prog;
    }
    return e;
}

// Lane 0's bounded wait until *flag == v, then the workgroup's acquire.
// false: the wait gave up (the communicator's sticky error is set).
__device__ __forceinline__ bool wait_flag(const uint64_t *flag, uint64_t v, int *err, uint64_t ticks) {
    __shared__ int ok;
    if (threadIdx.x == 0) {
        ok = 1;
        if (flag) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != v) {
                __builtin_amdgcn_s_sleep(1);
                if (__builtin_amdgcn_s_memrealtime() - t0 > ticks) {
                    __hip_atomic_store(err, (int)OMPI_AMD_ERR_TIMEOUT, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    ok = 0;
                    break;
                }
            }
        }
        sys_acquire();
    }
    __syncthreads();
    return ok != 0;
}

__global__ __launch_bounds__(kXferThreads) void eager_put_typed_kernel(typed_end te, int lds, char *typed,
                                                                       char *cell, int64_t bytes, int force64,
                                                                       uint64_t *flag, uint64_t v,
                                                                       uint64_t *mark, uint64_t mark_v) {
    __shared__ ddt_elem prog[kA2awLdsElems];
    const typed_end e = staged_end(te, prog, lds);
    typed_pipe_copy<false>(e, typed, cell, 0, bytes, bytes, false, force64 != 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        sys_release();
        __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (mark) __hip_atomic_store(mark, mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(kXferThreads) void eager_get_typed_kernel(typed_end te, int lds, const char *cell,
                                                                       char *typed, int64_t bytes, int force64,
                                                                       const uint64_t *flag, uint64_t v, int *err,
                                                                       uint64_t ticks, uint64_t *mark,
                                                                       uint64_t mark_v) {
    __shared__ ddt_elem prog[kA2awLdsElems];
    const typed_end e = staged_end(te, prog, lds);
    if (wait_flag(flag, v, err, ticks))
        typed_pipe_copy<true>(e, typed, const_cast<char *>(cell), 0, bytes, bytes, false, force64 != 0);
    xfer_epilogue();
    // the host's completion word (also after a timeout, as eager_get)
    if (threadIdx.x == 0 && mark) __hip_atomic_store(mark, mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(kXferThreads) void xfer_pack_sig_kernel(typed_end te, int lds, char *typed,
                                                                     char *stage, int64_t bytes, int force64,
                                                                     xfer_sig sg) {
    __shared__ ddt_elem prog[kA2awLdsElems];
    const typed_end e = staged_end(te, prog, lds);
    int64_t lo, hi;
    a2a_slice(bytes, (int)blockIdx.x, (int)gridDim.x, &lo, &hi);
    typed_pipe_copy<false>(e, typed, stage, lo, hi, bytes, true, force64 != 0);
    xfer_epilogue();  // this workgroup's stores released at system scope
    if (threadIdx.x != 0 || (!sg.flag && !sg.mark)) return;
    if (gridDim.x > 1) {  // the last workgroup to finish signals (xfer_copy_sig's rule)
        const uint32_t prev = __hip_atomic_fetch_add(sg.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
        if (prev != gridDim.x - 1) return;
        __hip_atomic_store(sg.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sys_release();
    }
    if (sg.flag) __hip_atomic_store(sg.flag, sg.flag_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (sg.mark) __hip_atomic_store(sg.mark, sg.mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(kXferThreads) void xfer_unpack_sig_kernel(typed_end te, int lds, const char *stage,
                                                                       char *typed, int64_t bytes, int force64,
                                                                       xfer_sig sg) {
    __shared__ ddt_elem prog[kA2awLdsElems];
    const typed_end e = staged_end(te, prog, lds);
    if (!wait_flag(sg.wait, sg.wait_v, sg.err, sg.ticks)) return;
    int64_t lo, hi;
    a2a_slice(bytes, (int)blockIdx.x, (int)gridDim.x, &lo, &hi);
    typed_pipe_copy<true>(e, typed, const_cast<char *>(stage), lo, hi, bytes, false, force64 != 0);
}

// Which of the two programs a two-ended launch stages in LDS (the host picks,
// the kernel obeys, the counters report).
enum { SR_LDS_SRC = 1, SR_LDS_DST = 2, SR_LDS_SAME = 4 };

// Every workgroup waits for sg.wait (none: only the acquire, after which a
// peer's program and buffer are read), stages the programs `lds` names —
// the source's at prog, the destination's behind it, or one copy for both
// when the two ends are one program — and moves its a2a_slice of the stream.
// The static LDS is xfer_unpack_sig_kernel's: kA2awLdsElems elements for the
// two programs together, so the occupancy is no worse than that kernel's.
__global__ __launch_bounds__(kXferThreads, 6) void ddt_sndrcv_kernel(typed_end se, typed_end re, int lds,
                                                                  const char *sbase, char *rbase, int64_t bytes,
                                                                  int force64, xfer_sig sg) {
    __shared__ ddt_elem prog[kA2awLdsElems];
    if (!wait_flag(sg.wait, sg.wait_v, sg.err, sg.ticks)) return;
    constexpr int W = (int)(sizeof(ddt_elem) / sizeof(uint64_t));
    typed_end s = se, r = re;
    if (lds & SR_LDS_SRC) {
        lds_words(prog, se.d.elems, se.d.nelem * W);
        s.d.elems = prog;
    }
    if (lds & SR_LDS_SAME) {
        r.d.elems = prog;
    } else if (lds & SR_LDS_DST) {
        ddt_elem *at = prog + ((lds & SR_LDS_SRC) ? se.d.nelem : 0);
        lds_words(at, re.d.elems, re.d.nelem * W);
        r.d.elems = at;
    }
    __syncthreads();
    int64_t lo, hi;
    a2a_slice(bytes, (int)blockIdx.x, (int)gridDim.x, &lo, &hi);
    typed_pipe_copy2(s, r, sbase, rbase, lo, hi, bytes, force64 != 0);
}

bool p2p_type_of(const ompi_amd_ddt_t *ddt, size_t *size) {
    ddt_view v;
    if (!ddt_view_of(ddt, &v) || v.d.nelem <= 0 || v.d.extent < 0 || v.d.size < 0) return false;
    *size = (size_t)v.d.size;
    return true;
}

// The launch's typed end, and what coll_typed.h's rule picks for it.
static typed_end launch_end(const ompi_amd_ddt_t *ddt, const void *typed, const void *contig, size_t bytes,
                            bool force64, int *lds, typed_pick *pick) {
    ddt_view v{};
    (void)ddt_view_of(ddt, &v);  // checked at the entry point (p2p_type_of)
    *lds = v.d.nelem <= kA2awLdsElems;
    pick->granule = typed_granule(v.gran, (uint64_t)(uintptr_t)typed, (uint64_t)(uintptr_t)contig);
    pick->lds = *lds != 0;
    pick->w64 = typed_walk64(bytes, pick->granule, force64);
    return end_of(true, v);
}

static unsigned typed_blocks(size_t bytes) {
    const int64_t per = (int64_t)kXferThreads * kDdtUnroll * 16;  // one pass of a workgroup at G = 16
    // persistent, under the byte copies' cap (one workgroup per CU, OMPI_AMD_OSC_MAX_BLOCKS)
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)bytes + per - 1) / per, osc_grid_cap()));
}

int eager_put_typed(const ompi_amd_ddt_t *ddt, const void *typed, char *cell, size_t bytes, bool force64,
                    uint64_t *flag, uint64_t v, uint64_t *mark, uint64_t mark_v, hipStream_t s,
                    typed_pick *pick) {
    int lds;
    const typed_end e = launch_end(ddt, typed, cell, bytes, force64, &lds, pick);
    hipLaunchKernelGGL(eager_put_typed_kernel, dim3(1), dim3(kXferThreads), 0, s, e, lds,
                       static_cast<char *>(const_cast<void *>(typed)), cell, (int64_t)bytes, force64 ? 1 : 0,
                       flag, v, mark, mark_v);
    return record_hip(hipGetLastError(), "p2p typed eager copy launch");
}

int eager_get_typed(const ompi_amd_ddt_t *ddt, const char *cell, void *typed, size_t bytes, bool force64,
                    const uint64_t *flag, uint64_t v, int *err, uint64_t ticks, uint64_t *mark,
                    uint64_t mark_v, hipStream_t s, typed_pick *pick) {
    int lds;
    const typed_end e = launch_end(ddt, typed, cell, bytes, force64, &lds, pick);
    hipLaunchKernelGGL(eager_get_typed_kernel, dim3(1), dim3(kXferThreads), 0, s, e, lds, cell,
                       static_cast<char *>(typed), (int64_t)bytes, force64 ? 1 : 0, flag, v, err, ticks, mark,
                       mark_v);
    return record_hip(hipGetLastError(), "p2p typed eager receive launch");
}

int xfer_pack_sig(const ompi_amd_ddt_t *ddt, const void *typed, void *stage, size_t bytes, bool force64,
                  hipStream_t s, const xfer_sig &sig, typed_pick *pick) {
    const unsigned blocks = typed_blocks(bytes);
    if (blocks > 1 && (sig.flag || sig.mark) && !sig.done) {
        record_msg("xfer_pack_sig: a multi-workgroup copy that signals needs a counter");
        return OMPI_AMD_ERR_BAD_PARAM;
    }
    int lds;
    const typed_end e = launch_end(ddt, typed, stage, bytes, force64, &lds, pick);
    hipLaunchKernelGGL(xfer_pack_sig_kernel, dim3(blocks), dim3(kXferThreads), 0, s, e, lds,
                       static_cast<char *>(const_cast<void *>(typed)), static_cast<char *>(stage),
                       (int64_t)bytes, force64 ? 1 : 0, sig);
    return record_hip(hipGetLastError(), "typed signalled pack launch");
}

int xfer_unpack_sig(const ompi_amd_ddt_t *ddt, const void *stage, void *typed, size_t bytes, bool force64,
                    hipStream_t s, const xfer_sig &sig, typed_pick *pick) {
    int lds;
    const typed_end e = launch_end(ddt, typed, stage, bytes, force64, &lds, pick);
    hipLaunchKernelGGL(xfer_unpack_sig_kernel, dim3(typed_blocks(bytes)), dim3(kXferThreads), 0, s, e, lds,
                       static_cast<const char *>(stage), static_cast<char *>(typed), (int64_t)bytes,
                       force64 ? 1 : 0, sig);
    return record_hip(hipGetLastError(), "typed signalled unpack launch");
}

bool typed_prog_of(const ompi_amd_ddt_t *ddt, typed_prog *out) {
    ddt_view v;
    if (!ddt_view_of(ddt, &v) || v.d.nelem <= 0 || v.d.extent < 0 || v.d.size <= 0) return false;
    out->elems = v.d.elems;
    out->nelem = v.d.nelem;
    out->gran = v.gran;
    out->size = v.d.size;
    out->extent = v.d.extent;
    return true;
}

static_assert(sizeof(ddt_elem) == kTypedElemBytes, "comm_internal.h's element size");

static typed_end end_of_prog(const typed_prog &p) {
    ddt_view v{};
    v.d = ddt_desc{static_cast<const ddt_elem *>(p.elems), p.nelem, p.size, p.extent, {0u, 0u, 0u}};
    v.gran = p.gran;
    return end_of(true, v);
}

int xfer_sndrcv(const typed_prog &sp, const void *sbase, const typed_prog &rp, void *rbase, size_t bytes,
                bool force64, hipStream_t s, const xfer_sig &sig, typed_pick *pick) {
    // both in LDS when they fit together (one copy when they are one program);
    // otherwise the larger one is walked from global memory
    const int ns = sp.nelem, nr = rp.nelem, K = kA2awLdsElems;
    int lds = 0;
    if (sp.elems == rp.elems) lds = ns <= K ? SR_LDS_SRC | SR_LDS_SAME : 0;
    else if (ns + nr <= K) lds = SR_LDS_SRC | SR_LDS_DST;
    else if (std::min(ns, nr) <= K) lds = ns <= nr ? SR_LDS_SRC : SR_LDS_DST;
    pick->granule = typed_granule2(sp.gran, rp.gran, (uint64_t)(uintptr_t)sbase, (uint64_t)(uintptr_t)rbase, 0);
    pick->lds = (lds & SR_LDS_SRC) && (lds & (SR_LDS_DST | SR_LDS_SAME));
    pick->w64 = typed_walk64_2(bytes, pick->granule, force64, (uint64_t)sp.size, (uint64_t)rp.size);
    hipLaunchKernelGGL(ddt_sndrcv_kernel, dim3(typed_blocks(bytes)), dim3(kXferThreads), 0, s, end_of_prog(sp),
                       end_of_prog(rp), lds, static_cast<const char *>(sbase), static_cast<char *>(rbase),
                       (int64_t)bytes, force64 ? 1 : 0, sig);
    return record_hip(hipGetLastError(), "typed-to-typed copy launch");
}

int xfer_pack_prog(const typed_prog &sp, const void *typed, void *dst, size_t bytes, bool force64, hipStream_t s,
                   typed_pick *pick) {
    const int lds = sp.nelem <= kA2awLdsElems;
    pick->granule = typed_granule(sp.gran, (uint64_t)(uintptr_t)typed, (uint64_t)(uintptr_t)dst);
    pick->lds = lds != 0;
    pick->w64 = typed_walk64(bytes, pick->granule, force64);
    hipLaunchKernelGGL(xfer_pack_sig_kernel, dim3(typed_blocks(bytes)), dim3(kXferThreads), 0, s,
                       end_of_prog(sp), lds, static_cast<char *>(const_cast<void *>(typed)),
                       static_cast<char *>(dst), (int64_t)bytes, force64 ? 1 : 0, xfer_sig{});
    return record_hip(hipGetLastError(), "typed pack launch (a peer's program)");
}

// ompi_amd_ddt_sndrcv_counts' slots, process-wide like the convertor's routes
static std::atomic<int64_t> g_sndrcv[OMPI_AMD_DDT_SNDRCV_SLOTS];
static std::atomic<int> g_sndrcv_force64{0};

}  // namespace ompi_amd

using namespace ompi_amd;

extern "C" {

int ompi_amd_ddt_sndrcv(const void *sbuf, size_t scount, const ompi_amd_ddt_t *sddt, void *rbuf, size_t rcount,
                        const ompi_amd_ddt_t *rddt, void *stream) {
    typed_prog sp, rp;
    size_t sbytes = 0, cap = 0;
    // a count of 0 ignores its datatype and its buffer
    const bool st = sddt && scount, rt = rddt && rcount;
    if ((st && !typed_prog_of(sddt, &sp)) || (rt && !typed_prog_of(rddt, &rp))) return OMPI_AMD_ERR_BAD_PARAM;
    if (__builtin_mul_overflow(scount, st ? (size_t)sp.size : 1, &sbytes) ||
        __builtin_mul_overflow(rcount, rt ? (size_t)rp.size : 1, &cap))
        return OMPI_AMD_ERR_BAD_PARAM;
    if ((sbytes && !sbuf) || (cap && !rbuf)) return OMPI_AMD_ERR_BAD_PARAM;
    if ((sbytes && !ompi_amd_is_device_pointer(sbuf)) || (cap && !ompi_amd_is_device_pointer(rbuf)))
        return OMPI_AMD_ERR_BAD_PARAM;
    int rc = OMPI_AMD_SUCCESS;
    size_t n = sbytes;
    if (n > cap) {  // ompi_datatype_sndrcv: what fits is copied, MPI_ERR_TRUNCATE
        n = cap;
        rc = OMPI_AMD_ERR_TRUNCATE;
        record_msg("ddt_sndrcv truncated: %zu bytes into %zu", sbytes, cap);
    }
    if (n == 0) return rc;
    const hipStream_t s = as_stream(stream);
    const bool force64 = g_sndrcv_force64.load(std::memory_order_relaxed) != 0;
    typed_pick pick;
    int lrc;
    if (st && rt) {
        lrc = xfer_sndrcv(sp, sbuf, rp, rbuf, n, force64, s, xfer_sig{}, &pick);
        g_sndrcv[OMPI_AMD_DDT_SNDRCV_LAUNCHES].fetch_add(1, std::memory_order_relaxed);
        g_sndrcv[OMPI_AMD_DDT_SNDRCV_BOTH_LDS].fetch_add(pick.lds ? 1 : 0, std::memory_order_relaxed);
        g_sndrcv[OMPI_AMD_DDT_SNDRCV_WALK64].fetch_add(pick.w64 ? 1 : 0, std::memory_order_relaxed);
        g_sndrcv[OMPI_AMD_DDT_SNDRCV_GRANULE].store(pick.granule, std::memory_order_relaxed);
    } else if (st) {
        lrc = xfer_pack_sig(sddt, sbuf, rbuf, n, force64, s, xfer_sig{}, &pick);
    } else if (rt) {
        lrc = xfer_unpack_sig(rddt, sbuf, rbuf, n, force64, s, xfer_sig{}, &pick);
    } else {
        lrc = record_hip(hipMemcpyAsync(rbuf, sbuf, n, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync (ddt_sndrcv)");
    }
    return lrc != OMPI_AMD_SUCCESS ? lrc : rc;
}

int ompi_amd_ddt_sndrcv_counts(int64_t *out, int n) {
    for (int i = 0; out && i < n && i < OMPI_AMD_DDT_SNDRCV_SLOTS; ++i)
        out[i] = g_sndrcv[i].load(std::memory_order_relaxed);
    return OMPI_AMD_DDT_SNDRCV_SLOTS;
}

void ompi_amd_ddt_sndrcv_force64(int on) { g_sndrcv_force64.store(on ? 1 : 0, std::memory_order_relaxed); }

}  // extern "C"
