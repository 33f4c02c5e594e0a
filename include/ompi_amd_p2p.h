/*
 * ompi_amd — point-to-point messages between device buffers of the ranks of
 * one node.  Replaces, for device memory, the PML
 * entry points (ompi/mca/pml/pml.h):
 *
 *   pml_isend  pml.h:317-326   pml_send   pml.h:341-349
 *   pml_irecv  pml.h:233-241   pml_recv   pml.h:262-270
 *   pml_iprobe pml.h:371-377   pml_probe  pml.h:398-403
 *
 * and the CUDA path underneath them: ob1's RDMA rendezvous for device
 * buffers (pml_ob1_cuda.c:56-101) over btl/smcuda, whose get copies from
 * the sender's buffer mapped with a CUDA IPC handle (btl_smcuda.c:1077-1250,
 * common_cuda.c:1008-1320).  Here the same receiver-driven "get" runs as
 * one copy kernel on the receiver's GPU that loads the sender's buffer
 * through its hipIpcOpenMemHandle mapping over xGMI; matching happens on
 * host in a POSIX shared-memory mailbox per (source, destination) pair
 * (created with the communicator), in MPI order: messages from one source
 * are matched in the order they were sent, receives in the order they were
 * posted, MPI_ANY_SOURCE / MPI_ANY_TAG as wildcards.
 *
 * Completion semantics.  A send's data is read in `stream` order (after
 * the work already queued on it).  Messages of at most 4 KiB (btl/smcuda's
 * eager limit) are copied into the sender's device eager area (ob1's eager
 * protocol): from a device buffer by a kernel on `stream` that publishes
 * the cell itself — the message is posted at once, the receiver's copy
 * waits for the cell on the device, and the send completes when that
 * kernel has run; from a host buffer before the call returns.  Larger ones
 * (after a synchronisation of `stream`) are copied into a library-owned
 * send stage (a pool of exported device buffers that live as long as the
 * communicator) and the send completes once staged — the receiver pulls
 * from the stage, so no peer ever maps an application buffer; MPI_Ssend
 * completes at the receiver's FIN.  Past the pool's cap (param
 * "p2p_stage_mib", default 1024) or with param "p2p_user_ipc" = 1 the
 * receiver maps the send buffer itself (rendezvous).  Host (pageable or
 * pinned) buffers are accepted on both sides: a host send always goes
 * through a stage, a host receive lands in a device receive stage and is
 * copied out before it completes.  MPI_Bsend is not provided.  A receive
 * completes when its data is in its buffer.  Host-side waits (a full
 * 64-slot ring, wait, probe) are bounded by param "p2p_timeout_ms" (-1: the
 * communicator's timeout_ms, the default; 0: no limit — the PML glue's
 * setting, MPI semantics).  The byte count is the message size.
 *
 * Derived datatypes.  The *_typed forms take a count of elements of an
 * ompi_amd_ddt_t (NULL: bytes) based at a device buffer, and the kernel that
 * moves the message walks the datatype: the sender packs straight into the
 * eager cell (at most 4 KiB packed) or a send stage, the receiver's copy-out
 * scatters into the receive layout.  On the wire a message
 * is its packed stream, so `bytes` in a status or a probe is packed bytes,
 * matching is unchanged, and a typed call on one side meets a byte call, or
 * a different datatype of the same packed length, on the other.
 *
 * Typed rendezvous.  A typed message to a peer that is
 * larger than 4 KiB packed and takes no stage goes out of the caller's buffer
 * as it lies: with "p2p_user_ipc" = 1 (a message of at most 4 KiB still goes
 * through the eager cell), or when the pool has no stage left.  The sender
 * copies its element program into the slot's eager cell, waits for the
 * buffer's producers, exports the allocation and posts; the receiver maps
 * buffer and program and runs one kernel that gathers through the sender's
 * datatype and scatters through its own (a byte receive: the one-ended pack
 * walk).  The send completes at the receiver's FIN.  It needs a program of at
 * most 39 elements (4 KiB of cell) and a buffer whose allocation peers can map
 * (an IPC-safe size, not older than an IPC close); without these a send under
 * "p2p_user_ipc" = 1 tries a stage, and a send that gets neither returns
 * OMPI_AMD_ERR_UNSUPPORTED before it took anything — the MCA glue then packs
 * non-contiguous datatypes first as it does for host buffers.  Messages to
 * self keep their behaviour exactly: a typed send to the own rank is refused
 * with OMPI_AMD_ERR_UNSUPPORTED under "p2p_user_ipc" = 1 and when the pool has
 * no stage left.
 */
#ifndef OMPI_AMD_P2P_H
#define OMPI_AMD_P2P_H

#include <stddef.h>
#include <stdint.h>

#include "ompi_amd_coll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OMPI_AMD_ANY_SOURCE (-1)     /* MPI_ANY_SOURCE */
#define OMPI_AMD_ANY_TAG    (-1)     /* MPI_ANY_TAG */
#define OMPI_AMD_ERR_TRUNCATE (-7)   /* message longer than the receive buffer */

/* mca_pml_base_send_mode_t, same values (pml_constants.h:30-37) */
#define OMPI_AMD_SEND_SYNCHRONOUS 0
#define OMPI_AMD_SEND_COMPLETE    1
#define OMPI_AMD_SEND_BUFFERED    2
#define OMPI_AMD_SEND_READY       3
#define OMPI_AMD_SEND_STANDARD    4

typedef struct ompi_amd_p2p_request ompi_amd_p2p_request_t;

/* ompi_status_public_t's fields (MPI_SOURCE, MPI_TAG, MPI_ERROR, count). */
typedef struct {
    int source;
    int tag;
    int error;
    size_t bytes;
} ompi_amd_status_t;

/* Nonblocking send of `bytes` from `buf` (device or host memory) to rank
 * `dst`.  tag >= 0.  Up to 64 sends to one destination may be unmatched at
 * a time; the 65th waits (bounded by p2p_timeout_ms) for one to
 * complete. */
int ompi_amd_isend(ompi_amd_comm_t *comm, const void *buf, size_t bytes, int dst, int tag,
                   int mode, void *stream, ompi_amd_p2p_request_t **request);
/* Nonblocking receive into `buf` (device or host) of capacity `bytes` from
 * `src` (or OMPI_AMD_ANY_SOURCE) with `tag` (or OMPI_AMD_ANY_TAG).  The
 * copy runs on `stream` once the message is matched. */
int ompi_amd_irecv(ompi_amd_comm_t *comm, void *buf, size_t bytes, int src, int tag,
                   void *stream, ompi_amd_p2p_request_t **request);
/* Blocking forms: isend/irecv + wait + free. */
int ompi_amd_send(ompi_amd_comm_t *comm, const void *buf, size_t bytes, int dst, int tag,
                  int mode, void *stream);
int ompi_amd_recv(ompi_amd_comm_t *comm, void *buf, size_t bytes, int src, int tag,
                  void *stream, ompi_amd_status_t *status);
/* MPI_Sendrecv: both posted before either is waited on. */
int ompi_amd_sendrecv(ompi_amd_comm_t *comm, const void *sbuf, size_t sbytes, int dst, int stag,
                      void *rbuf, size_t rbytes, int src, int rtag, void *stream,
                      ompi_amd_status_t *status);
/* The same calls for `count` elements of `ddt` based at the device buffer
 * `buf` (ddt NULL: count bytes).  `ddt` is kept by reference until the
 * request completes.  A message shorter than the receive writes exactly its
 * bytes of the stream (it may end inside an element) and nothing else; bytes
 * the datatype does not own are never written.  OMPI_AMD_ERR_BAD_PARAM, with
 * no request, for what the byte forms refuse, a host buffer, a datatype
 * without a device program or with a negative extent, and count * size past
 * SIZE_MAX.  Counters (get_param): p2p_typed_eager, p2p_typed_staged (sends
 * by path), p2p_typed_recv (receives whose copy-out walked a datatype),
 * p2p_typed_lds (those with the program in LDS), p2p_typed_granule (access
 * width of the last typed launch), p2p_typed_walk64 (typed launches that ran
 * the 64-bit walk; "typed_force64" forces it), p2p_typed_rndv (sends that
 * went by typed rendezvous; they count in neither p2p_typed_staged nor
 * p2p_typed_eager), p2p_typed_sndrcv (receives that ran the kernel with a
 * datatype on both ends; they count in p2p_typed_recv too, and in
 * p2p_typed_lds when both programs were in LDS).  A typed staged send does not
 * count in p2p_staged_sends.  sendrecv_typed posts its receive only once its
 * send can no longer be refused: after OMPI_AMD_ERR_UNSUPPORTED it has
 * matched no message. */
int ompi_amd_isend_typed(ompi_amd_comm_t *comm, const void *buf, size_t count,
                         const ompi_amd_ddt_t *ddt, int dst, int tag, int mode, void *stream,
                         ompi_amd_p2p_request_t **request);
int ompi_amd_irecv_typed(ompi_amd_comm_t *comm, void *buf, size_t count, const ompi_amd_ddt_t *ddt,
                         int src, int tag, void *stream, ompi_amd_p2p_request_t **request);
int ompi_amd_send_typed(ompi_amd_comm_t *comm, const void *buf, size_t count,
                        const ompi_amd_ddt_t *ddt, int dst, int tag, int mode, void *stream);
int ompi_amd_recv_typed(ompi_amd_comm_t *comm, void *buf, size_t count, const ompi_amd_ddt_t *ddt,
                        int src, int tag, void *stream, ompi_amd_status_t *status);
int ompi_amd_sendrecv_typed(ompi_amd_comm_t *comm, const void *sbuf, size_t scount,
                            const ompi_amd_ddt_t *sddt, int dst, int stag, void *rbuf, size_t rcount,
                            const ompi_amd_ddt_t *rddt, int src, int rtag, void *stream,
                            ompi_amd_status_t *status);
/* *done = 1 when complete (status filled for receives; status may be NULL).
 * Every test / wait also matches pending receives of the communicator. */
int ompi_amd_p2p_test(ompi_amd_p2p_request_t *request, int *done, ompi_amd_status_t *status);
int ompi_amd_p2p_wait(ompi_amd_p2p_request_t *request, ompi_amd_status_t *status);
/* Waits for completion, then releases the request. */
int ompi_amd_p2p_free(ompi_amd_p2p_request_t *request);
/* MPI_Iprobe / MPI_Probe: a message that a receive with (src, tag) would
 * match, without receiving it. */
int ompi_amd_iprobe(ompi_amd_comm_t *comm, int src, int tag, int *flag, ompi_amd_status_t *status);
int ompi_amd_probe(ompi_amd_comm_t *comm, int src, int tag, ompi_amd_status_t *status);

#ifdef __cplusplus
}
#endif

#endif /* OMPI_AMD_P2P_H */
