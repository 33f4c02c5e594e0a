// Device side of the xGMI collectives (coll_ipc.hip): the shared job and
// pointer-set types, the memory-ordering helpers, the reduction fold in the
// reference algorithms' operand orders, and the reduce / fused-allreduce
// kernel templates.  The kernels are instantiated per op by coll_kern.hip
// (one object per op, compiled in parallel) and reached through the
// per-op launch rows declared at the end.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ompi_amd_coll.h"
#include "coll_typed.h"
#include "ddt_device.h"
#include "op_device.h"

namespace ompi_amd {

constexpr int kMaxRanks = OMPI_AMD_MAX_RANKS;
constexpr int kXferThreads = 256;

struct ptr_set { const char *p[kMaxRanks]; };
struct flag_set { uint64_t *p[kMaxRanks]; };

// Operand orders of the reference's reduction algorithms.  Sources are
// loaded in virtual-rank order v[j] = x[(first + j) % n].
enum order_t {
    ORDER_RING = 0,      // ring / ring_segmented block `first`; linear scan (first 0)
    ORDER_TREE = 1,      // recursive doubling (first 0)
    ORDER_CHAIN = 2,     // pipeline chain rooted at `first`; basic_linear = chain at 0, no swap
    ORDER_BINOMIAL = 3,  // in-order binomial tree rooted at `first`
    ORDER_BINARY = 4,    // binary tree rooted at `first`
    ORDER_HALVING = 5,   // recursive-halving reduce_scatter, owner tmp rank in flags >> 8
    ORDER_RABEN = 6,     // Rabenseifner allreduce (redscat_allgather), owner vrank in flags >> 8
};
// The root passed MPI_IN_PLACE: its first combine is f(own, child)
// (coll_base_reduce.c:170-171, 196-199).
constexpr int FOLD_ROOT_INPLACE = 1;
// Launch flag, not a fold rule: the vector body stores non-temporally
// (param "copy_nt", the 8-GPU bench's A/B; fold() never reads bit 16).
constexpr int FOLD_NT_STORE = 1 << 16;

// One reduction job: elements [off, off+cnt) of every source, combined in
// the call's order and written to dst + off_dst (element units).
struct red_job {
    int64_t off, cnt, off_dst;
    int first;  // virtual rank 0 (ring block b, tree root)
    int head;   // elements before the 16-B aligned body; -1: no common alignment
    int aux = 0;  // per-job fold flags, or-ed into the launch's (ORDER_RABEN: owner vrank << 8)
};
// a ring block cut at the Rabenseifner pieces: up to kMaxRanks + 1 jobs
struct red_jobs { red_job j[2 * kMaxRanks]; int n; };

struct cp_job { const char *src; char *dst; int64_t bytes; };
struct cp_jobs { cp_job j[kMaxRanks]; int n; };

// the acquiring lane waits for its invalidate before the barrier that
// lets the other waves load (Guideline 16: the fence itself does not wait)
__device__ __forceinline__ void sys_acquire() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void sys_release() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The workgroup's acquire: lane 0 issues it (it invalidates the CU's L1 and
// the XCD's L2 for every wave of the CU), the barrier holds the other waves
// until it completed.  One per workgroup instead of one per wave: in a
// 1024-workgroup grid the 4 per workgroup cost measurable bandwidth
// (osc_ipc.hip's grid note).
__device__ __forceinline__ void acquire_once() {
    if (threadIdx.x == 0) sys_acquire();
    __syncthreads();
}

// Wait until *flag >= epoch (a peer's barrier store).  Bounded: past
// `ticks` (s_memrealtime, 100 MHz) the communicator's sticky error word (host
// memory, written only — a spinning wave never reads host memory) is set and
// the communicator's abort word (in its own flag page, device memory) is
// raised.  Every ~1 ms of waiting the abort word is read, so once any wait
// of this communicator has given up — or a failing peer raised the word
// (abort_peers) — every later wait gives up within 1 ms: a rank whose peer
// failed a call it had already launched drains its queued collectives in one
// timeout instead of one per barrier, and reaches comm_destroy's host
// rendezvous while that peer is still there to keep its memory alive.
// Returns false when the wait gave up.
// The flag page: 32 rows x 16 ranks of epochs (4 KiB), then the abort word.
constexpr int kAbortWord = 512;               // uint64 index in the flag page
constexpr size_t kFlagPageBytes = 8192;

// seen (debug, OMPI_AMD_DEBUG_PROGRESS=1; else null): the flag value read
// at every ~1 ms check, in host-mapped memory a watchdog can print.
__device__ __forceinline__ bool wait_epoch(const uint64_t *flag, uint64_t epoch, int *err,
                                           uint64_t ticks, uint64_t *abort_word,
                                           uint64_t *seen = nullptr) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t check = t0 + 100000;  // 1 ms
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
        __builtin_amdgcn_s_sleep(1);
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (now - t0 > ticks) {
            __hip_atomic_store(err, (int)OMPI_AMD_ERR_TIMEOUT, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(abort_word, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        if (now >= check) {
            if (seen)
                __hip_atomic_store(seen, __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (__hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
                __hip_atomic_store(err, (int)OMPI_AMD_ERR_TIMEOUT, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
                return false;
            }
            check = now + 100000;
        }
    }
    return true;
}

// Every storing wave drains its stores before the workgroup's single
// system-scope release (MI355X_MICROARCH.md, inter-workgroup visibility).
__device__ __forceinline__ void xfer_epilogue() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) sys_release();
}

// ---------------------------------------------------------------- reduce
// Fold v[0..n) (virtual-rank order) with the 2-buffer rule f(out, in).  All
// array indices are compile-time constants after unrolling; n, order and
// flags are wave-uniform.
template <typename T, int OP, int NM = kMaxRanks>
__device__ __forceinline__ T fold(const T (&v)[NM], int n, int order, int flags) {
    using F = opfn<OP, false>;
    const bool swap = (flags & FOLD_ROOT_INPLACE) != 0;
    if (order == ORDER_RING) {
        // v[j] = x[(b + j) % n]; acc = x[b]; acc = f(x[b+j], acc)
        T acc = v[0];
#pragma unroll
        for (int j = 1; j < NM; ++j)
            if (j < n) acc = F::template f<T>(v[j], acc);
        return acc;
    }
    if (order == ORDER_CHAIN) {
        // chain fanout 1 (coll_base_topo.c:588-600) under the generic reduce
        // (coll_base_reduce.c:206-215): node k's only child is k+1,
        // acc_k = f(acc_(k+1), x_k); basic_linear (:680-721) is the same
        // expression at first = 0.
        T acc = v[NM - 1];
#pragma unroll
        for (int j = NM - 1; j >= 0; --j) {
            if (j == n - 1) acc = v[j];
            else if (j < n - 1) acc = (j == 0 && swap) ? F::template f<T>(v[0], acc)
                                                       : F::template f<T>(acc, v[j]);
        }
        return acc;
    }
    if (order == ORDER_BINOMIAL) {
        // in-order binomial (coll_base_topo.c:402-458): vrank u's children
        // are u+1, u+2, u+4, ... while the bit is clear; first child:
        // acc = f(child, own), later ones acc = f(acc, child).
        T w[NM];
#pragma unroll
        for (int i = 0; i < NM; ++i) w[i] = v[i];
#pragma unroll
        for (int u = 0; u + 1 < NM; u += 2)
            if (u + 1 < n) w[u] = (u == 0 && swap) ? F::template f<T>(w[0], w[1])
                                                   : F::template f<T>(w[u + 1], w[u]);
#pragma unroll
        for (int m = 2; m < NM; m <<= 1) {
#pragma unroll
            for (int u = 0; u + m < NM; u += 2 * m)
                if (u + m < n) w[u] = F::template f<T>(w[u], w[u + m]);
        }
        return w[0];
    }
    if (order == ORDER_BINARY) {
        // build_tree(2) (coll_base_topo.c:77-175): shifted rank s has
        // children s + d and s + 2d, d = largest power of two <= s + 1;
        // children have larger s, so descending s sees them finished.
        T w[NM];
#pragma unroll
        for (int i = 0; i < NM; ++i) w[i] = v[i];
#pragma unroll
        for (int s = NM - 1; s >= 0; --s) {
            int d = 1;
            while (2 * d <= s + 1) d *= 2;
            const int c0 = s + d, c1 = s + 2 * d;
            if (c0 < NM && c0 < n)
                w[s] = (s == 0 && swap) ? F::template f<T>(w[0], w[c0])
                                        : F::template f<T>(w[c0], w[s]);
            if (c1 < NM && c1 < n) w[s] = F::template f<T>(w[s], w[c1]);
        }
        return w[0];
    }
    if (order == ORDER_RABEN) {
        // redscat_allgather (coll_base_allreduce.c:970-1243).  Step 1: the
        // 2*rem lowest ranks pair up; the even one keeps the left half of
        // the vector as f(even, odd), the odd one the right half as
        // f(odd, even) (:1031-1080) — the owner's bit 0 says which half
        // this element is in.  Step 2: recursive halving over the p' vranks
        // with masks 1, 2, 4, ... (:1122-1171): at every mask the vrank
        // keeping the element's part does f(mine, partner's).  o = the
        // vrank the element ends on.
        int adj = 1;
        while (adj * 2 <= n) adj *= 2;
        const int rem = n - adj;
        const int o = (flags >> 8) & 0xff;
        const bool right = (o & 1) != 0;
        T w[NM];
#pragma unroll
        for (int u = 0; u < NM; ++u) {
            if (2 * u + 1 < NM && u < rem)
                w[u] = right ? F::template f<T>(v[2 * u + 1], v[2 * u])
                             : F::template f<T>(v[2 * u], v[2 * u + 1]);
            else if (u < adj)
                w[u] = v[u + rem < NM ? u + rem : 0];
        }
#pragma unroll
        for (int m = 1; m < NM; m <<= 1) {
            if (m < adj) {
#pragma unroll
                for (int u = 0; u < NM; ++u)
                    if (u < adj && (u & m) == (o & m)) w[u] = F::template f<T>(w[u], w[u ^ m]);
            }
        }
        T r = w[0];
#pragma unroll
        for (int u = 1; u < NM; ++u)
            if (u == o) r = w[u];
        return r;
    }
    if (order == ORDER_HALVING) {
        // recursive-halving reduce_scatter (coll_base_reduce_scatter.c:
        // 203-345): the 2*remain lowest ranks fold pairwise (odd keeps:
        // f(odd, even)), then at every mask from the top the rank holding
        // the owner's half does f(mine, partner's).  tb = the owner's tmp
        // rank; holders at mask m agree with tb on bit m, and their
        // partners never do, so the update can run in place.
        int adj = 1;
        while (adj * 2 <= n) adj *= 2;
        const int remain = n - adj;
        const int tb = (flags >> 8) & 0xff;
        T w[NM];
#pragma unroll
        for (int u = 0; u < NM; ++u) {
            if (2 * u + 1 < NM && u < remain) w[u] = F::template f<T>(v[2 * u + 1], v[2 * u]);
            else if (u < adj) w[u] = v[u + remain];
        }
#pragma unroll
        for (int m = NM / 2; m >= 1; m >>= 1) {
            if (m < adj) {
#pragma unroll
                for (int u = 0; u < NM; ++u)
                    if (u < adj && (u & m) == (tb & m)) w[u] = F::template f<T>(w[u], w[u ^ m]);
            }
        }
        T r = w[0];
#pragma unroll
        for (int u = 1; u < NM; ++u)
            if (u == tb) r = w[u];
        return r;
    }
    // recursive doubling (coll_base_allreduce.c:184-236): fold the
    // 2*extra lowest ranks pairwise, then a pairwise tree; every combine is
    // f(out = higher, in = lower).
    int adj = 1;
    while (adj * 2 <= n) adj *= 2;
    const int extra = n - adj;
    T w[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        if (i < extra) w[i] = F::template f<T>(v[2 * i + 1], v[2 * i]);
        else if (i < adj) w[i] = v[i + extra];
    }
#pragma unroll
    for (int len = NM; len > 1; len >>= 1) {
        if (len <= adj) {
#pragma unroll
            for (int i = 0; i < NM / 2; ++i)
                if (2 * i + 1 < len) w[i] = F::template f<T>(w[2 * i + 1], w[2 * i]);
        }
    }
    return w[0];
}

// Gather v[j] for element index e of the sources in virtual-rank order.
template <typename T, int NM = kMaxRanks>
__device__ __forceinline__ void gather_scalar(T (&v)[NM], const ptr_set &src, int n,
                                              int first, int64_t e) {
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        if (j < n) {
            const int r = (first + j) % n;
            v[j] = reinterpret_cast<const T *>(src.p[r])[e];
        }
    }
}

// NM: the register arrays' size, a compile-time bound >= n (8 for up to 8
// ranks, else 16: at N <= 8 the kernel holds half the vectors, 109 -> fewer
// VGPRs and more waves per SIMD).
// n sources (virtual ranks 0..n), result stored to dst.p[0 .. ndst): ndst =
// 1 is a plain reduce into one buffer; ndst = size is the fused push of the
// owner's block into every rank's rbuf (the host orders dst local first,
// then peers rank+1, rank+2, ... so concurrent owners spread their stores
// over the links).
template <typename T, int OP, int NM = kMaxRanks>
__global__ __launch_bounds__(kXferThreads) void reduce_kernel(ptr_set src, ptr_set dst, int ndst,
                                                              int n, int order, int flags,
                                                              red_jobs jobs) {
    acquire_once();
    const red_job jb = jobs.j[blockIdx.y];
    constexpr int E = 16 / sizeof(T);
    const int64_t gstride = (int64_t)gridDim.x * kXferThreads;
    const int64_t tid = (int64_t)blockIdx.x * kXferThreads + threadIdx.x;
    // vector body [head, head + nvec*E): every source and dst 16-B aligned
    // there (head < 0: no common alignment, all scalar)
    const int64_t head = jb.head < 0 ? jb.cnt : jb.head;
    const int64_t nvec = jb.head < 0 ? 0 : (jb.cnt - head) / E;
    for (int64_t i = tid; i < nvec; i += gstride) {
        vec16<T> v[NM];
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            if (j < n) {
                const int r = (jb.first + j) % n;
                const u32x4 *p = reinterpret_cast<const u32x4 *>(
                    reinterpret_cast<const T *>(src.p[r]) + jb.off + head);
                v[j].v = __builtin_nontemporal_load(p + i);
            }
        }
        vec16<T> out;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            T s[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) s[j] = v[j].e[e];
            out.e[e] = fold<T, OP, NM>(s, n, order, flags | jb.aux);
        }
        if (flags & FOLD_NT_STORE) {
#pragma unroll
            for (int k = 0; k < NM; ++k)
                if (k < ndst)
                    __builtin_nontemporal_store(
                        out.v, reinterpret_cast<u32x4 *>(reinterpret_cast<T *>(const_cast<char *>(dst.p[k])) +
                                                         jb.off_dst + head) + i);
        } else {
#pragma unroll
            for (int k = 0; k < NM; ++k)
                if (k < ndst)
                    reinterpret_cast<u32x4 *>(reinterpret_cast<T *>(const_cast<char *>(dst.p[k])) +
                                              jb.off_dst + head)[i] = out.v;
        }
    }
    // scalar head [0, head) and tail [head + nvec*E, cnt)
    const int64_t tail0 = head + nvec * E;
    const int64_t nscalar = head + (jb.cnt - tail0);
    for (int64_t k = tid; k < nscalar; k += gstride) {
        const int64_t e = k < head ? k : tail0 + (k - head);
        T s[NM];
        gather_scalar<T, NM>(s, src, n, jb.first, jb.off + e);
        const T r = fold<T, OP, NM>(s, n, order, flags | jb.aux);
#pragma unroll
        for (int d = 0; d < NM; ++d)
            if (d < ndst)
                store_elem<T>(reinterpret_cast<T *>(const_cast<char *>(dst.p[d])) + jb.off_dst + e,
                              r);
    }
    xfer_epilogue();
}

// ---------------------------------------------------------------- fused small allreduce
// One launch for small messages (param "fused_bytes"): every workgroup
// stages its slice of my input in my scratch half, signals the peers on its
// own flag row, waits for the same slice of every peer and folds it.
// Workgroup g depends only on the peers' workgroup g (same slice), so there
// is no grid-wide sync.  Flag slot [g * kMaxRanks + p] of rank r holds the
// last epoch peer p's workgroup g signalled to r (row 0 doubles as the
// barrier kernel's row; epochs only grow, so the users never collide).
constexpr int kFusedMaxGroups = 4096 / (int)sizeof(uint64_t) / kMaxRanks;  // 32 rows

struct fused_args {
    const char *src;
    char *dst, *mine;
    ptr_set peers;
    uint64_t *flags;
    flag_set peer_flags;
    int rank, n, order;
    int64_t count, split, early, late;
    uint64_t epoch, timeout_ticks;
    int *err;
    // ompi_amd_allreduce_wait: the last workgroup to finish stores mark_v
    // into the pinned host word `mark` (done: a zeroed counter in my flag
    // page) — the host's wait needs no mark kernel after this one
    uint32_t *done;
    uint64_t *mark;
    uint64_t mark_v;
};

// flag-page word (uint32 index) of the fused kernel's finished-workgroup counter
constexpr int kFusedDoneWord = 8192 / (int)sizeof(uint32_t);
// completion counters of fused launches that store their own mark: slot k
// at word kFusedDoneWord + kFusedDoneStride * k (own 64-B line), slot 0 the
// blocking call's, the others persistent plans' (up to kPipeFlagOff)
constexpr int kFusedDoneStride = 64 / (int)sizeof(uint32_t);
constexpr int kFusedDoneSlots = (64 << 10) / 64 - 8192 / 64;

template <typename T, int OP>
__global__ __launch_bounds__(kXferThreads) void fused_allreduce_kernel(fused_args a) {
    const int t = threadIdx.x;
    const int g = blockIdx.y * gridDim.x + blockIdx.x;
    int64_t off = 0, cnt = a.count;
    int first = 0;
    if (a.order == ORDER_RING) {  // grid row y = ring block y
        const int64_t b = blockIdx.y;
        off = b < a.split ? b * a.early : b * a.late + a.split;
        cnt = b < a.split ? a.early : a.late;
        first = (int)b;
    }
    const int64_t per = (cnt + gridDim.x - 1) / gridDim.x;
    const int64_t lo = off + min(cnt, per * (int64_t)blockIdx.x);
    const int64_t hi = off + min(cnt, per * (int64_t)(blockIdx.x + 1));
    const T *src = reinterpret_cast<const T *>(a.src);
    T *mine = reinterpret_cast<T *>(a.mine);
    for (int64_t e = lo + t; e < hi; e += kXferThreads) mine[e] = src[e];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) sys_release();
    __syncthreads();
    __shared__ int gave_up;
    if (t == 0) gave_up = 0;
    __syncthreads();
    if (t < a.n && t != a.rank) {
        __hip_atomic_store(a.peer_flags.p[t] + g * kMaxRanks + a.rank, a.epoch, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        if (!wait_epoch(a.flags + g * kMaxRanks + t, a.epoch, a.err, a.timeout_ticks,
                        a.flags + kAbortWord))
            gave_up = 1;
    }
    __syncthreads();
    if (gave_up) return;  // a peer never arrived: its scratch is not ours to read
    acquire_once();
    T *dst = reinterpret_cast<T *>(a.dst);
    for (int64_t e = lo + t; e < hi; e += kXferThreads) {
        T v[kMaxRanks];
        gather_scalar<T>(v, a.peers, a.n, first, e);
        store_elem<T>(dst + e, fold<T, OP>(v, a.n, a.order, 0));
    }
    if (a.mark) {  // the host-observed completion, by the last workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // my results, device-wide
            const uint32_t total = gridDim.x * gridDim.y;
            if (__hip_atomic_fetch_add(a.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == total - 1) {
                __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.mark, a.mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ---------------------------------------------------------------- pipelined large allreduce
// The two-shot schemes' three phases — send (C: my input's blocks to where
// their owners fold them), fold (F: the owner folds its block and stores the
// result where the others gather it), gather (G: the other blocks into my
// rbuf) — in ONE launch with per-slice flags instead of a device barrier
// between phases.  Every block is cut into slices; workgroup w owns slices
// w, w + G, w + 2G, ... of every block, and at its iteration p it runs C of
// its slice p, F of slice p - 1 and G of slice p - 2, then drains its
// stores, releases once, and tells every peer "C(p) and F(p - 1) done" on
// its own flag row.  Before iteration p it waits only for the SAME
// workgroup of every peer to have finished iteration p - 1 (its C(p - 1)
// feeds my F(p - 1), its F(p - 2) my G(p - 2)): no grid-wide sync, and
// copy, fold and gather traffic of different slices is in flight together
// (the staging copy of pull, the scatter of push, overlap the transfers
// instead of preceding them behind a barrier).  Which buffers the phases
// touch is the host's choice (coll_ipc.hip: staged pull, push-gather,
// push-land).  Element e of the vector sits at p + e * sizeof(T) for every
// pointer below (the host biases landing-slot pointers by their block's
// offset).  Flag rows live kPipeFlagOff bytes into each rank's flag
// allocation: [phase C / F][workgroup][peer] of uint64 counters,
// (seq << 20) + (iterations done), seq the same on every rank per call.
constexpr int kPipeMaxGroups = 1024;
constexpr size_t kPipeFlagOff = 64 << 10;
constexpr size_t kPipeFlagBytes = 2 * (size_t)kPipeMaxGroups * kMaxRanks * sizeof(uint64_t);

struct pipe_args {
    const char *src;
    ptr_set dst_c;  // per block: where C sends it (null: not sent — my own block)
    ptr_set src_f;  // per rank: the fold's sources (virtual order from `first`)
    ptr_set dst_f;  // the fold's destinations [0, ndst)
    ptr_set src_g;  // per block: where G gathers it from (null: not gathered)
    char *rbuf;
    uint64_t *flags;      // my pipe rows
    flag_set peer_flags;  // every peer's pipe rows as mapped here
    int rank, n, mine, ndst, order, first, fold_flags, nt;
    int colocated;  // most ranks of this communicator sharing one GPU (co-residency cap)
    int64_t split, early, late;  // ring blocks (blockcount)
    int64_t per, nslices;        // elements per slice (a multiple of 16 B), slices per block
    uint64_t seq, timeout_ticks;
    int *err;
    uint64_t *abort_word;
};

__device__ __forceinline__ size_t pipe_row(int phase, int w, int r) {
    return ((size_t)phase * kPipeMaxGroups + (size_t)w) * kMaxRanks + (size_t)r;
}

// Bytes [lo, hi) from s to d by one workgroup: 16-B vectors, 4 in flight
// per lane, when s and d share their phase mod 16; else bytewise.
__device__ __forceinline__ void pipe_copy(const char *s, char *d, int64_t lo, int64_t hi, bool nt) {
    const int t = threadIdx.x;
    if (hi <= lo) return;
    int64_t head = hi - lo, nv = 0;
    if ((((uintptr_t)(s + lo) ^ (uintptr_t)(d + lo)) & 15) == 0) {
        head = min(hi - lo, (int64_t)((16 - ((uintptr_t)(s + lo) & 15)) & 15));
        nv = (hi - lo - head) / 16;
    }
    const u32x4 *sv = reinterpret_cast<const u32x4 *>(s + lo + head);
    u32x4 *dv = reinterpret_cast<u32x4 *>(d + lo + head);
    constexpr int S = kXferThreads;
    int64_t i = t;
    for (; i + 3 * S < nv; i += 4 * S) {
        const u32x4 a = __builtin_nontemporal_load(sv + i);
        const u32x4 b = __builtin_nontemporal_load(sv + i + S);
        const u32x4 c = __builtin_nontemporal_load(sv + i + 2 * S);
        const u32x4 e = __builtin_nontemporal_load(sv + i + 3 * S);
        if (nt) {
            __builtin_nontemporal_store(a, dv + i);
            __builtin_nontemporal_store(b, dv + i + S);
            __builtin_nontemporal_store(c, dv + i + 2 * S);
            __builtin_nontemporal_store(e, dv + i + 3 * S);
        } else {
            dv[i] = a;
            dv[i + S] = b;
            dv[i + 2 * S] = c;
            dv[i + 3 * S] = e;
        }
    }
    for (; i < nv; i += S) {
        if (nt) __builtin_nontemporal_store(__builtin_nontemporal_load(sv + i), dv + i);
        else dv[i] = __builtin_nontemporal_load(sv + i);
    }
    const int64_t tail0 = lo + head + nv * 16;
    const int64_t nrest = head + (hi - tail0);
    for (int64_t k = t; k < nrest; k += S) {
        const int64_t b = k < head ? lo + k : tail0 + (k - head);
        d[b] = s[b];
    }
}

// Elements [lo, hi) of the fold by one workgroup (reduce_kernel's body).
template <typename T, int OP, int NM>
__device__ __forceinline__ void pipe_fold(const pipe_args &a, int64_t lo, int64_t hi) {
    constexpr int E = 16 / sizeof(T);
    const int t = threadIdx.x;
    if (hi <= lo) return;
    // vector body where every source and destination is 16-B aligned
    const uintptr_t ph = (uintptr_t)(a.dst_f.p[0] + lo * (int64_t)sizeof(T)) & 15;
    bool same = true;
#pragma unroll
    for (int j = 0; j < NM; ++j)
        if (j < a.n) same = same && (((uintptr_t)(a.src_f.p[j] + lo * (int64_t)sizeof(T)) & 15) == ph);
#pragma unroll
    for (int k = 1; k < NM; ++k)
        if (k < a.ndst) same = same && (((uintptr_t)(a.dst_f.p[k] + lo * (int64_t)sizeof(T)) & 15) == ph);
    const int64_t lead = (int64_t)((16 - ph) & 15);
    int64_t head = hi - lo, nv = 0;
    if (same && lead % (int64_t)sizeof(T) == 0) {
        head = min(hi - lo, lead / (int64_t)sizeof(T));
        nv = (hi - lo - head) / E;
    }
    const int64_t v0 = lo + head;
    for (int64_t i = t; i < nv; i += kXferThreads) {
        vec16<T> v[NM];
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            if (j < a.n) {
                const int r = (a.first + j) % a.n;
                const u32x4 *p = reinterpret_cast<const u32x4 *>(reinterpret_cast<const T *>(a.src_f.p[r]) + v0);
                v[j].v = __builtin_nontemporal_load(p + i);
            }
        }
        vec16<T> out;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            T s[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) s[j] = v[j].e[e];
            out.e[e] = fold<T, OP, NM>(s, a.n, a.order, a.fold_flags);
        }
#pragma unroll
        for (int k = 0; k < NM; ++k) {
            if (k < a.ndst) {
                u32x4 *q = reinterpret_cast<u32x4 *>(reinterpret_cast<T *>(const_cast<char *>(a.dst_f.p[k])) + v0) + i;
                if (a.nt) __builtin_nontemporal_store(out.v, q);
                else *q = out.v;
            }
        }
    }
    const int64_t tail0 = v0 + nv * E;
    const int64_t nrest = head + (hi - tail0);
    for (int64_t k = t; k < nrest; k += kXferThreads) {
        const int64_t e = k < head ? lo + k : tail0 + (k - head);
        T s[NM];
        gather_scalar<T, NM>(s, a.src_f, a.n, a.first, e);
        const T r = fold<T, OP, NM>(s, a.n, a.order, a.fold_flags);
#pragma unroll
        for (int d = 0; d < NM; ++d)
            if (d < a.ndst) store_elem<T>(reinterpret_cast<T *>(const_cast<char *>(a.dst_f.p[d])) + e, r);
    }
}

template <typename T, int OP, int NM>
__global__ __launch_bounds__(kXferThreads) void pipe_allreduce_kernel(pipe_args a) {
    const int t = threadIdx.x, w = blockIdx.x, G = gridDim.x;
    const int64_t P = (a.nslices - w + G - 1) / G;  // my slices (the host sizes G <= nslices)
    constexpr int64_t ext = sizeof(T);
    __shared__ int gave_up;
    if (t == 0) gave_up = 0;
    __syncthreads();
    for (int64_t p = 0; p < P + 2; ++p) {
        const bool doC = p < P, doF = p >= 1 && p <= P, doG = p >= 2;
        if (p >= 1) {
            if (t < a.n && t != a.rank) {
                bool ok = true;
                if (doF)  // peer t's C(p - 1): its share of my block's slice p - 1
                    ok = wait_epoch(a.flags + pipe_row(0, w, t), a.seq + (uint64_t)p, a.err,
                                    a.timeout_ticks, a.abort_word);
                if (ok && doG)  // peer t's F(p - 2): its block's slice p - 2 folded
                    ok = wait_epoch(a.flags + pipe_row(1, w, t), a.seq + (uint64_t)(p - 1), a.err,
                                    a.timeout_ticks, a.abort_word);
                if (!ok) gave_up = 1;
            }
            __syncthreads();
            if (gave_up) return;  // a peer never arrived: its memory is not ours to read
            acquire_once();
        }
        if (doC) {
            const int64_t s = w + p * G;
#pragma unroll
            for (int b = 0; b < NM; ++b) {
                if (b >= a.n || !a.dst_c.p[b]) continue;
                const int64_t off = b < a.split ? b * a.early : b * a.late + a.split;
                const int64_t cnt = b < a.split ? a.early : a.late;
                const int64_t lo = off + min(cnt, s * a.per), hi = off + min(cnt, (s + 1) * a.per);
                pipe_copy(a.src, const_cast<char *>(a.dst_c.p[b]), lo * ext, hi * ext, a.nt);
            }
        }
        if (doF) {
            const int64_t s = w + (p - 1) * G;
            const int b = a.mine;
            const int64_t off = b < a.split ? b * a.early : b * a.late + a.split;
            const int64_t cnt = b < a.split ? a.early : a.late;
            pipe_fold<T, OP, NM>(a, off + min(cnt, s * a.per), off + min(cnt, (s + 1) * a.per));
        }
        if (doG) {
            const int64_t s = w + (p - 2) * G;
#pragma unroll
            for (int b = 0; b < NM; ++b) {
                if (b >= a.n || !a.src_g.p[b]) continue;
                const int64_t off = b < a.split ? b * a.early : b * a.late + a.split;
                const int64_t cnt = b < a.split ? a.early : a.late;
                const int64_t lo = off + min(cnt, s * a.per), hi = off + min(cnt, (s + 1) * a.per);
                pipe_copy(a.src_g.p[b], a.rbuf, lo * ext, hi * ext, a.nt);
            }
        }
        if (doC || doF) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t == 0) sys_release();
            __syncthreads();
            if (t < a.n && t != a.rank) {
                if (doC)
                    __hip_atomic_store(a.peer_flags.p[t] + pipe_row(0, w, a.rank), a.seq + (uint64_t)(p + 1),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (doF)
                    __hip_atomic_store(a.peer_flags.p[t] + pipe_row(1, w, a.rank), a.seq + (uint64_t)p,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    xfer_epilogue();
}

// ---------------------------------------------------------------- fused small alltoall(v)
// One launch for small personalised exchanges (param "fused_bytes"), on the
// fused allreduce's protocol and flag rows: workgroup g STORES its slice of
// every block of my send buffer into the receiver's scratch half, slot
// [me] (a remote store: posted writes, no round trip per access; the
// allgather's landing path moves its data the same way), drains its stores,
// releases at system scope and signals every peer on flag row g; it then
// waits for workgroup g of every peer, acquires, and copies the same slice
// of every slot of MY scratch half into rbuf.  Workgroup g depends only on
// the peers' workgroup g.  The slice of block p -> q is cut from values p
// and q hold alike: the grid (from the call's agreed largest pair) and the
// pair's byte count.  Counts and displacements are bytes; block p -> q sits
// in its slot at phase sphase[q] (on p) == rphase[p] (on q) mod 16, so both
// copies run as 16-B vectors whenever their two ends share that phase.
struct a2a_args {
    const char *sbuf;
    char *rbuf, *mine;   // mine: my scratch half (slot [p] holds what p sent me)
    ptr_set peers;       // every rank's scratch half as mapped here
    uint64_t *flags;
    flag_set peer_flags;
    int rank, n;
    int self_copy;       // 0: in place, my own block stays where it is
    int64_t slot;        // bytes per slot
    int64_t scount[kMaxRanks], sdispl[kMaxRanks], rcount[kMaxRanks], rdispl[kMaxRanks];
    uint8_t sphase[kMaxRanks], rphase[kMaxRanks];
    uint64_t epoch, timeout_ticks;
    int *err;
    // host-observed completion by the last workgroup (fused_args)
    uint32_t *done;
    uint64_t *mark;
    uint64_t mark_v;
};

// bytes [*lo, *hi) of a b-byte block that workgroup g of G moves (16-B granules)
__host__ __device__ __forceinline__ void a2a_slice(int64_t b, int g, int G, int64_t *lo, int64_t *hi) {
    const int64_t per = ((b + G - 1) / G + 15) & ~(int64_t)15;
    *lo = per * g < b ? per * g : b;
    *hi = per * (g + 1) < b ? per * (g + 1) : b;
}

template <bool NT>
__global__ __launch_bounds__(kXferThreads) void fused_alltoall_kernel(a2a_args a) {
    const int t = threadIdx.x, g = blockIdx.x, G = gridDim.x;
    int64_t lo, hi;
    for (int k = 0; k < a.n; ++k) {  // my own block first, then peers rank+1, rank+2, ...
        const int q = (a.rank + k) % a.n;
        if (k == 0 && !a.self_copy) continue;
        a2a_slice(a.scount[q], g, G, &lo, &hi);
        char *d = k == 0 ? a.rbuf + a.rdispl[q]
                         : const_cast<char *>(a.peers.p[q]) + (int64_t)a.rank * a.slot + a.sphase[q];
        pipe_copy(a.sbuf + a.sdispl[q], d, lo, hi, NT && k != 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) sys_release();
    __syncthreads();
    __shared__ int gave_up;
    if (t == 0) gave_up = 0;
    __syncthreads();
    if (t < a.n && t != a.rank) {
        __hip_atomic_store(a.peer_flags.p[t] + g * kMaxRanks + a.rank, a.epoch, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        if (!wait_epoch(a.flags + g * kMaxRanks + t, a.epoch, a.err, a.timeout_ticks,
                        a.flags + kAbortWord))
            gave_up = 1;
    }
    __syncthreads();
    if (gave_up) return;  // a peer never arrived: its slot holds nothing of this call
    acquire_once();
    for (int p = 0; p < a.n; ++p) {
        if (p == a.rank) continue;
        a2a_slice(a.rcount[p], g, G, &lo, &hi);
        pipe_copy(a.mine + (int64_t)p * a.slot + a.rphase[p], a.rbuf + a.rdispl[p], lo, hi, false);
    }
    if (a.mark) {  // the host-observed completion, by the last workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (__hip_atomic_fetch_add(a.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
                (uint32_t)G - 1) {
                __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.mark, a.mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ---------------------------------------------------------------- fused small allgatherv
// The alltoall kernel above with every send displacement equal would read my
// block once per destination.  This one runs on the same protocol, flag rows
// and a2a_args (scount / sdispl[rank] describe my block; sphase[rank] is its
// phase in the peers' slots), but workgroup g LOADS each 16-B vector of its
// slice once and STORES it to my own rbuf position (unless in place) and to
// slot [me] of every peer's scratch half, peers in the order me+1, me+2, ...
// That needs the source and every destination at one phase mod 16; if they
// are not, each destination gets its own pipe_copy, as in the alltoall.
// The second half — drain, barrier, one release, signal, wait, acquire, copy
// the slots out, mark — is the alltoall kernel's, statement for statement.
template <bool NT>
__global__ __launch_bounds__(kXferThreads) void fused_allgatherv_kernel(a2a_args a) {
    const int t = threadIdx.x, g = blockIdx.x, G = gridDim.x;
    int64_t lo, hi;
    a2a_slice(a.scount[a.rank], g, G, &lo, &hi);
    if (hi > lo) {
        const char *s = a.sbuf + a.sdispl[a.rank];
        char *own = a.rbuf + a.rdispl[a.rank];
        const int64_t at = (int64_t)a.rank * a.slot + a.sphase[a.rank];  // my block in a peer's half
        const uintptr_t ph = (uintptr_t)(s + lo) & 15;
        bool same = !a.self_copy || ((uintptr_t)(own + lo) & 15) == ph;
        for (int k = 1; k < a.n; ++k)
            same = same && ((uintptr_t)(a.peers.p[(a.rank + k) % a.n] + at + lo) & 15) == ph;
        if (same) {
            const int64_t head = min(hi - lo, (int64_t)((16 - ph) & 15));
            const int64_t nv = (hi - lo - head) / 16;
            const int64_t body = lo + head;
            const u32x4 *sv = reinterpret_cast<const u32x4 *>(s + body);
            constexpr int S = kXferThreads;
            int64_t i = t;
            for (; i + 3 * S < nv; i += 4 * S) {  // 4 loads in flight per lane, as pipe_copy
                const u32x4 v0 = __builtin_nontemporal_load(sv + i);
                const u32x4 v1 = __builtin_nontemporal_load(sv + i + S);
                const u32x4 v2 = __builtin_nontemporal_load(sv + i + 2 * S);
                const u32x4 v3 = __builtin_nontemporal_load(sv + i + 3 * S);
                if (a.self_copy) {
                    u32x4 *dv = reinterpret_cast<u32x4 *>(own + body);
                    dv[i] = v0;
                    dv[i + S] = v1;
                    dv[i + 2 * S] = v2;
                    dv[i + 3 * S] = v3;
                }
                for (int k = 1; k < a.n; ++k) {
                    u32x4 *dv = reinterpret_cast<u32x4 *>(
                        const_cast<char *>(a.peers.p[(a.rank + k) % a.n]) + at + body);
                    if (NT) {
                        __builtin_nontemporal_store(v0, dv + i);
                        __builtin_nontemporal_store(v1, dv + i + S);
                        __builtin_nontemporal_store(v2, dv + i + 2 * S);
                        __builtin_nontemporal_store(v3, dv + i + 3 * S);
                    } else {
                        dv[i] = v0;
                        dv[i + S] = v1;
                        dv[i + 2 * S] = v2;
                        dv[i + 3 * S] = v3;
                    }
                }
            }
            for (; i < nv; i += S) {
                const u32x4 v = __builtin_nontemporal_load(sv + i);
                if (a.self_copy) reinterpret_cast<u32x4 *>(own + body)[i] = v;
                for (int k = 1; k < a.n; ++k) {
                    u32x4 *dv = reinterpret_cast<u32x4 *>(
                        const_cast<char *>(a.peers.p[(a.rank + k) % a.n]) + at + body);
                    if (NT) __builtin_nontemporal_store(v, dv + i);
                    else dv[i] = v;
                }
            }
            // the bytes before and after the vector body
            const int64_t tail0 = body + nv * 16;
            const int64_t nrest = head + (hi - tail0);
            for (int64_t r = t; r < nrest; r += S) {
                const int64_t b = r < head ? lo + r : tail0 + (r - head);
                const char v = s[b];
                if (a.self_copy) own[b] = v;
                for (int k = 1; k < a.n; ++k)
                    const_cast<char *>(a.peers.p[(a.rank + k) % a.n])[at + b] = v;
            }
        } else {
            if (a.self_copy) pipe_copy(s, own, lo, hi, false);
            for (int k = 1; k < a.n; ++k)
                pipe_copy(s, const_cast<char *>(a.peers.p[(a.rank + k) % a.n]) + at, lo, hi, NT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) sys_release();
    __syncthreads();
    __shared__ int gave_up;
    if (t == 0) gave_up = 0;
    __syncthreads();
    if (t < a.n && t != a.rank) {
        __hip_atomic_store(a.peer_flags.p[t] + g * kMaxRanks + a.rank, a.epoch, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        if (!wait_epoch(a.flags + g * kMaxRanks + t, a.epoch, a.err, a.timeout_ticks,
                        a.flags + kAbortWord))
            gave_up = 1;
    }
    __syncthreads();
    if (gave_up) return;  // a peer never arrived: its slot holds nothing of this call
    acquire_once();
    for (int p = 0; p < a.n; ++p) {
        if (p == a.rank) continue;
        a2a_slice(a.rcount[p], g, G, &lo, &hi);
        pipe_copy(a.mine + (int64_t)p * a.slot + a.rphase[p], a.rbuf + a.rdispl[p], lo, hi, false);
    }
    if (a.mark) {  // the host-observed completion, by the last workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (__hip_atomic_fetch_add(a.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
                (uint32_t)G - 1) {
                __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.mark, a.mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ---------------------------------------------------------------- typed exchange
// One end of an exchange copy that walks a derived datatype (ddt_device.h):
// the program, its granule, and size / G as a multiply-high divisor for
// every G the walk may pick.  d.elems == nullptr: the end is plain bytes.
struct typed_end {
    ddt_desc d;
    fastdiv sdiv[5];  // size / G for G = 1, 2, 4, 8, 16 (where G divides the size and it fits 32 bits)
    int gran;
};

// ng G-byte granules from stream byte lo on: `typed` is the typed base of the
// block, `contig` the address of stream byte lo.  kDdtUnroll typed addresses
// first, then as many independent loads in flight, then the stores
// (ddt_kernels.hip's ddt_body, by one workgroup).
template <int G, bool UNPACK>
__device__ __forceinline__ void typed_walk(const typed_end &e, char *typed, char *contig, int64_t lo,
                                           int64_t ng, bool nt, bool w64) {
    using T = typename granule<G>::t;
    constexpr int U = kDdtUnroll, S = kXferThreads;
    constexpr int LG = G == 16 ? 4 : G == 8 ? 3 : G == 4 ? 2 : G == 2 ? 1 : 0;
    const ddt_elem *el = e.d.elems;
    const int n = e.d.nelem;
    const uint32_t size_g = (uint32_t)(e.d.size >> LG);
    const fastdiv sdiv = e.sdiv[LG];
    const T *cs = reinterpret_cast<const T *>(contig);
    T *cd = reinterpret_cast<T *>(contig);
    for (int64_t j0 = threadIdx.x; j0 < ng; j0 += (int64_t)S * U) {
        int64_t toff[U];
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = j0 + u * S;
            if (j < ng)
                toff[u] = w64 ? typed_offset<int64_t>(el, n, e.d.size, e.d.extent, lo + j * G)
                              : typed_offset_fast<G>(el, n, size_g, sdiv, e.d.extent,
                                                     (uint32_t)((lo >> LG) + j));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = j0 + u * S;
            if (j < ng)
                v[u] = UNPACK ? __builtin_nontemporal_load(cs + j)
                              : *reinterpret_cast<const T *>(typed + toff[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = j0 + u * S;
            if (j < ng) {
                if (UNPACK) *reinterpret_cast<T *>(typed + toff[u]) = v[u];
                else if (nt) __builtin_nontemporal_store(v[u], cd + j);
                else cd[j] = v[u];
            }
        }
    }
}

// Packed-stream bytes [lo, hi) of a pair of `pair` packed bytes, by one
// workgroup: between the typed layout of e based at `typed` and contiguous
// memory whose stream byte 0 is at `contig` (UNPACK: contiguous -> typed).
// nt: the contiguous end is a peer's memory, store non-temporally.  The
// granule and the walk are coll_typed.h's rule; lo enters the granule beside
// the contiguous address, so a range cut anywhere is still moved by aligned
// accesses (the engine cuts at multiples of 16).  Bytes past the last whole
// granule — none when [lo, hi) ends on an element or a 16-B cut — go bytewise.
template <bool UNPACK>
__device__ __forceinline__ void typed_pipe_copy(const typed_end &e, char *typed, char *contig, int64_t lo,
                                                int64_t hi, int64_t pair, bool nt, bool force64) {
    if (hi <= lo) return;
    char *c = contig + lo;
    const int G = typed_granule(e.gran, (uint64_t)(uintptr_t)typed, (uint64_t)(uintptr_t)c | (uint64_t)lo);
    const int64_t ng = (hi - lo) / G;
    const bool w64 = typed_walk64((uint64_t)pair, G, force64);
    switch (G) {
    case 16: typed_walk<16, UNPACK>(e, typed, c, lo, ng, nt, w64); break;
    case 8: typed_walk<8, UNPACK>(e, typed, c, lo, ng, nt, w64); break;
    case 4: typed_walk<4, UNPACK>(e, typed, c, lo, ng, nt, w64); break;
    case 2: typed_walk<2, UNPACK>(e, typed, c, lo, ng, nt, w64); break;
    default: typed_walk<1, UNPACK>(e, typed, c, lo, ng, nt, w64); break;
    }
    for (int64_t p = lo + ng * G + threadIdx.x; p < hi; p += kXferThreads) {
        const int64_t t = typed_offset<int64_t>(e.d.elems, e.d.nelem, e.d.size, e.d.extent, p);
        if (UNPACK) typed[t] = contig[p];
        else contig[p] = typed[t];
    }
}

// copy_kernel's job table with an optional datatype on one end of a job:
// job blockIdx.y moves stream bytes [lo, hi) of its pair, workgroup
// blockIdx.x the a2a_slice of them.  A typed end is the block's typed base,
// a contiguous end the address of stream byte 0.  (Both ends typed never
// meet in one job: such a block goes through a slot, §3.5.)
enum { TCP_BYTES = 0, TCP_SRC_TYPED = 1, TCP_DST_TYPED = 2 };
struct tcp_job {
    const char *src;
    char *dst;
    int64_t lo, hi, pair;
    int typed;  // TCP_*
};
struct tcp_jobs {
    tcp_job j[kMaxRanks];
    int n;
    int force64;
    typed_end se, re;  // the send datatype (TCP_SRC_TYPED), the receive datatype (TCP_DST_TYPED)
};

template <bool NT>
__global__ __launch_bounds__(kXferThreads) void typed_copy_kernel(tcp_jobs jobs) {
    acquire_once();
    const tcp_job jb = jobs.j[blockIdx.y];
    int64_t lo, hi;
    a2a_slice(jb.hi - jb.lo, (int)blockIdx.x, (int)gridDim.x, &lo, &hi);
    lo += jb.lo;
    hi += jb.lo;
    if (jb.typed == TCP_SRC_TYPED)
        typed_pipe_copy<false>(jobs.se, const_cast<char *>(jb.src), jb.dst, lo, hi, jb.pair, NT,
                               jobs.force64 != 0);
    else if (jb.typed == TCP_DST_TYPED)
        typed_pipe_copy<true>(jobs.re, jb.dst, const_cast<char *>(jb.src), lo, hi, jb.pair, false,
                              jobs.force64 != 0);
    else
        pipe_copy(jb.src, jb.dst, lo, hi, NT);
    xfer_epilogue();
}

// fused_alltoall_kernel with typed ends: workgroup g moves packed bytes
// a2a_slice(count, g, G) of every block, reading the send layout on the way
// out and writing the receive layout on the way in; a slot holds the packed
// stream at phase 0.  My own block goes directly when at most one side is
// typed, and through my own slot [me] when both are.  The protocol — drain,
// barrier, one system release, signal on row g, wait_epoch, one acquire,
// copy-out, embedded host mark — is the byte kernel's, statement for
// statement.
struct typed_a2a_args {
    a2a_args a;
    typed_end se, re;
    int force64;
};

template <bool NT>
__global__ __launch_bounds__(kXferThreads) void fused_alltoall_typed_kernel(typed_a2a_args ta) {
    const a2a_args &a = ta.a;
    const int t = threadIdx.x, g = blockIdx.x, G = gridDim.x;
    const bool st = ta.se.d.elems != nullptr, rt = ta.re.d.elems != nullptr;
    const bool f64 = ta.force64 != 0;
    int64_t lo, hi;
    for (int k = 0; k < a.n; ++k) {  // my own block first, then peers rank+1, rank+2, ...
        const int q = (a.rank + k) % a.n;
        if (k == 0 && !a.self_copy) continue;
        a2a_slice(a.scount[q], g, G, &lo, &hi);
        const bool direct = k == 0 && !(st && rt);
        char *s = const_cast<char *>(a.sbuf) + a.sdispl[q];
        char *d = direct ? a.rbuf + a.rdispl[q]
                         : (k == 0 ? a.mine : const_cast<char *>(a.peers.p[q])) + (int64_t)a.rank * a.slot;
        if (st) typed_pipe_copy<false>(ta.se, s, d, lo, hi, a.scount[q], NT && k != 0, f64);
        else if (direct && rt) typed_pipe_copy<true>(ta.re, d, s, lo, hi, a.scount[q], false, f64);
        else pipe_copy(s, d, lo, hi, NT && k != 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) sys_release();
    __syncthreads();
    __shared__ int gave_up;
    if (t == 0) gave_up = 0;
    __syncthreads();
    if (t < a.n && t != a.rank) {
        __hip_atomic_store(a.peer_flags.p[t] + g * kMaxRanks + a.rank, a.epoch, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        if (!wait_epoch(a.flags + g * kMaxRanks + t, a.epoch, a.err, a.timeout_ticks,
                        a.flags + kAbortWord))
            gave_up = 1;
    }
    __syncthreads();
    if (gave_up) return;  // a peer never arrived: its slot holds nothing of this call
    acquire_once();
    for (int p = 0; p < a.n; ++p) {
        if (p == a.rank && !(a.self_copy && st && rt)) continue;
        a2a_slice(a.rcount[p], g, G, &lo, &hi);
        char *s = a.mine + (int64_t)p * a.slot;
        if (rt) typed_pipe_copy<true>(ta.re, a.rbuf + a.rdispl[p], s, lo, hi, a.rcount[p], false, f64);
        else pipe_copy(s, a.rbuf + a.rdispl[p], lo, hi, false);
    }
    if (a.mark) {  // the host-observed completion, by the last workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (__hip_atomic_fetch_add(a.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
                (uint32_t)G - 1) {
                __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.mark, a.mark_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ---------------------------------------------------------------- launch rows
using red_launch_fn = hipError_t (*)(dim3, const ptr_set &, const ptr_set &, int, int, int, int,
                                     const red_jobs &, hipStream_t);
using fused_launch_fn = hipError_t (*)(dim3, const fused_args &, hipStream_t);
using pipe_launch_fn = hipError_t (*)(unsigned, const pipe_args &, hipStream_t);

// Row `op` of the launch tables: OMPI_AMD_TYPE_COUNT entries, NULL where
// op/base has no handler (slot_supported).  Defined by coll_kern.hip built
// once per op with -DCOLL_OP=<op>.
#define OMPI_AMD_COLL_OPS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
#define OMPI_AMD_COLL_ROW_DECL(k)          \
    const red_launch_fn *red_row_##k();    \
    const fused_launch_fn *fused_row_##k(); \
    const pipe_launch_fn *pipe_row_##k();
OMPI_AMD_COLL_OPS(OMPI_AMD_COLL_ROW_DECL)
#undef OMPI_AMD_COLL_ROW_DECL

}  // namespace ompi_amd
