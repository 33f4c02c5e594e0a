// Landing-buffer layouts of the collectives (host only, plain values).  Post,
// persistent init and launch all take slot stride, result offset and byte
// need from here, so a deferred call's launch never grows the buffer its
// post sized (tests/harness/landing_layout_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ompi_amd {

// Largest allocation the library exports or maps: on ROCm 7.2
// hipIpcOpenMemHandle of a 2 GiB + 2 MiB allocation never returned (four
// ranks on one MI355X, OMPI_AMD_TRACE=1); 1 GiB opened in < 1 ms.
constexpr size_t kMaxIpcBytes = (2ull << 30) - (4u << 20);
// an allgather / bcast landing need this close to the cap keeps the handle swap
constexpr size_t kLandCapMargin = 64u << 20;

// slot: stride of the per-sender input slots; result_off: the end of the
// input slots, where the result area starts; need: usable landing bytes.
// blk: the bcast's block; land: push-land rather than push-gather.
struct land_layout {
    size_t slot, result_off, need, blk;
    bool land;
};

inline size_t land_round(size_t x) { return (x + 255) & ~(size_t)255; }
// a slot of `bytes` at any phase mod 16 B
inline size_t ag_land_slot(size_t bytes) { return land_round(bytes + 16); }
// the largest block of `count` elements cut into n (blockcount's early)
inline size_t land_early(size_t count, int n) { return (count + (size_t)n - 1) / (size_t)n; }
// need, or 0 when it is too close to the IPC cap for the landing path
inline size_t land_capped(size_t need) { return need + kLandCapMargin <= kMaxIpcBytes ? need : 0; }

// push allreduce: slot r of the owner's buffer holds rank r's copy of the
// owner's block (results go to the peers' rbufs)
inline land_layout push_landing(int n, size_t count, size_t ext) {
    const size_t slot = ag_land_slot(land_early(count, n) * ext);
    return {slot, slot * (size_t)n, slot * (size_t)n, 0, false};
}
// Staged push allreduce: push-gather adds its result slot [n]; push-land n
// result slots (one per block), falling back to push-gather when 2n slots
// would pass the IPC size limit (every rank computes the same).
inline land_layout staged_push_landing(int n, size_t count, size_t ext, bool want_land) {
    land_layout l = push_landing(n, count, ext);
    l.land = want_land && l.slot * (size_t)(2 * n) <= kMaxIpcBytes;
    l.need = l.slot * (size_t)(l.land ? 2 * n : n + 1);
    return l;
}
// reduce: push's slots, and the whole result behind them (used at the root)
inline land_layout reduce_landing(int n, size_t count, size_t ext) {
    land_layout l = push_landing(n, count, ext);
    l.need += land_round(count * ext);
    return l;
}
// reduce_scatter(_block): n input slots of the largest block, result slot [n]
inline land_layout reduce_scatter_landing(int n, size_t max_cnt, size_t ext) {
    const size_t slot = ag_land_slot(max_cnt * ext);
    return {slot, slot * (size_t)n, slot * (size_t)(n + 1), 0, false};
}
// reduce_scatter over exported buffers, some rank in place: the result alone
inline land_layout reduce_scatter_inplace_landing(size_t max_cnt, size_t ext) {
    return {0, 0, max_cnt * ext + 256, 0, false};
}
// scan / exscan: this rank's input, once
inline land_layout scan_landing(size_t bytes) { return {bytes + 256, bytes + 256, bytes + 256, 0, false}; }
// allgather: rank p's block in slot p
inline land_layout allgather_landing(int n, size_t bytes) {
    const size_t slot = ag_land_slot(bytes);
    return {slot, slot * (size_t)n, land_capped(slot * (size_t)n), 0, false};
}
// the block of a scatter + allgather bcast
inline size_t bcast_block(int n, size_t bytes) { return land_round((bytes + (size_t)n - 1) / (size_t)n); }
// bcast: the buffer mirrored (offset o at offset o), moved in n blocks
inline land_layout bcast_landing(int n, size_t bytes) {
    const size_t all = land_round(bytes) + 256;
    return {all, all, land_capped(all), bcast_block(n, bytes), false};
}
// alltoall: n slots of one pass (`chunk` bytes per pair, or the largest pair M)
inline land_layout alltoall_landing(int n, size_t chunk, size_t M) {
    const size_t slot = ag_land_slot(std::min(chunk, M));
    return {slot, slot * (size_t)n, slot * (size_t)n, 0, false};
}
// the largest chunk whose n alltoall slots fit `avail` bytes (0: not even 256 B)
inline size_t alltoall_fit_chunk(int n, size_t avail) {
    const size_t per = (avail / (size_t)n) & ~(size_t)255;
    return per < 512 ? 0 : per - 256;
}
// allgatherv / gather(v) / scatter(v) ride the alltoall's exchange.  `slots`
// says how many senders store into one rank's landing buffer in a pass: all
// n for allgatherv and gather(v) (slot [p] holds rank p's block), ONE for
// scatter(v) (only the root stores, into slot [0]).  need = slots * slot.
inline land_layout exchange_landing(int slots, size_t chunk, size_t M) {
    return alltoall_landing(slots, chunk, M);
}
inline int allgatherv_slots(int n) { return n; }
inline int gather_slots(int n) { return n; }
inline int scatter_slots(int /*n*/) { return 1; }
inline land_layout allgatherv_landing(int n, size_t chunk, size_t M) {
    return exchange_landing(allgatherv_slots(n), chunk, M);
}
inline land_layout gather_landing(int n, size_t chunk, size_t M) {
    return exchange_landing(gather_slots(n), chunk, M);
}
inline land_layout scatter_landing(int n, size_t chunk, size_t M) {
    return exchange_landing(scatter_slots(n), chunk, M);
}

}  // namespace ompi_amd
