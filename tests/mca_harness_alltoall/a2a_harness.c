/*
 * TEST HARNESS ONLY.  One rank of a multi-process run that drives the
 * alltoall / alltoallv slots of ompi_amd/mca/coll/rocm/coll_rocm_module.c
 * the way the coll framework does: the previously selected functions are
 * recording stand-ins, the component is queried, the module enabled (it
 * saves and retains the stand-ins) and its six functions installed in the
 * communicator's table; every call then goes through that table.
 *
 *   CPU (HARNESS_GPU=0): the module offers the six slots.
 *   GPU (HARNESS_GPU=1): device buffers take the device path (no saved call,
 *   exact results, int counts and element displacements converted to bytes);
 *   host buffers reach the saved function as host pointers; a rank whose send
 *   and receive byte counts differ reaches it too; under the DEVICE lock a
 *   vector-typed send operand (2 doubles every 4) is packed and exact, for
 *   alltoall and for alltoallv (displacements in extents of that type);
 *   ialltoallv and a persistent alltoall complete through their requests;
 *   release drops every reference enable took.
 *
 * usage: a2a_harness <segment-name> <rank> <size>; prints "ok" / "ok gpu".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mpi.h"
#include "ompi/communicator/communicator.h"
#include "ompi/constants.h"
#include "ompi/datatype/ompi_datatype.h"
#include "ompi/op/op.h"
#include "ompi/runtime/ompi_rte.h"
#include "opal/runtime/opal_progress.h"
#include "coll_rocm.h"
#include "ompi_amd.h"

extern mca_coll_rocm_component_t mca_coll_rocm_component;
extern int harness_dev_alloc_copy(void **d, const void *h, size_t bytes);
extern int harness_dev_copy_back(void *h, const void *d, size_t bytes);
extern int harness_dev_free(void *d);

OBJ_CLASS_INSTANCE(mca_coll_base_module_t, opal_object_t, NULL, NULL);
harness_proc_name_t harness_proc_name = {4243, 0};
int ompi_op_ddt_map[64];
struct ompi_datatype_t harness_mpi_byte = {2, 1, 1, 1};

static int g_rank, g_size;
#define CHECK(c, ...)                                                   \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAIL rank %d %s:%d: ", g_rank, __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                               \
            fprintf(stderr, "\n");                                      \
            exit(1);                                                    \
        }                                                               \
    } while (0)

/* every slot of the table: the module's enable saves them all */
#define OTHER_SLOTS(X)                                                                         \
    X(allgather) X(allreduce) X(bcast) X(exscan) X(reduce) X(reduce_scatter)                   \
    X(reduce_scatter_block) X(scan) X(iallgather) X(iallreduce) X(ibcast)                      \
    X(ireduce_scatter_block) X(iexscan) X(ireduce) X(ireduce_scatter) X(iscan)                 \
    X(allgather_init) X(allreduce_init) X(bcast_init) X(reduce_scatter_block_init)             \
    X(exscan_init) X(reduce_init) X(reduce_scatter_init) X(scan_init)
#define A2A_SLOTS(X) X(alltoall) X(alltoallv) X(ialltoall) X(ialltoallv) X(alltoall_init) X(alltoallv_init)

/* ---- the recording saved functions: which one ran, and on what memory ---- */
static int saved_calls[2];  /* alltoall, alltoallv */
static int saved_dev;       /* a saved function was handed a device pointer */

static void note(int which, const void *s, const void *r)
{
    ++saved_calls[which];
    if ((NULL != s && MPI_IN_PLACE != s && ompi_amd_is_device_pointer(s)) ||
        (NULL != r && ompi_amd_is_device_pointer(r)))
        ++saved_dev;
}

static int sv_alltoall(const void *s, int sc, struct ompi_datatype_t *sd, void *r, int rc,
                       struct ompi_datatype_t *rd, struct ompi_communicator_t *c,
                       mca_coll_base_module_t *m)
{
    note(0, s, r);
    return OMPI_SUCCESS;
}
static int sv_alltoallv(const void *s, const int *sc, const int *sdp, struct ompi_datatype_t *sd,
                        void *r, const int *rc, const int *rdp, struct ompi_datatype_t *rd,
                        struct ompi_communicator_t *c, mca_coll_base_module_t *m)
{
    note(1, s, r);
    return OMPI_SUCCESS;
}
static int sv_ialltoall(const void *s, int sc, struct ompi_datatype_t *sd, void *r, int rc,
                        struct ompi_datatype_t *rd, struct ompi_communicator_t *c,
                        ompi_request_t **rq, mca_coll_base_module_t *m)
{
    return OMPI_ERROR;  /* not reached in this harness */
}
static int sv_ialltoallv(const void *s, const int *sc, const int *sdp, struct ompi_datatype_t *sd,
                         void *r, const int *rc, const int *rdp, struct ompi_datatype_t *rd,
                         struct ompi_communicator_t *c, ompi_request_t **rq,
                         mca_coll_base_module_t *m)
{
    return OMPI_ERROR;
}
static int sv_alltoall_init(const void *s, int sc, struct ompi_datatype_t *sd, void *r, int rc,
                            struct ompi_datatype_t *rd, struct ompi_communicator_t *c,
                            struct ompi_info_t *info, ompi_request_t **rq, mca_coll_base_module_t *m)
{
    return OMPI_ERROR;
}
static int sv_alltoallv_init(const void *s, const int *sc, const int *sdp, struct ompi_datatype_t *sd,
                             void *r, const int *rc, const int *rdp, struct ompi_datatype_t *rd,
                             struct ompi_communicator_t *c, struct ompi_info_t *info,
                             ompi_request_t **rq, mca_coll_base_module_t *m)
{
    return OMPI_ERROR;
}

/* ---- data: element i of block p -> q (exact in float and double) ---- */
static double val(int p, int q, size_t i, int salt)
{
    return (double) (p * 4096 + q * 256 + salt * 16) + (double) (i % 1024) * 0.25;
}

static void *dev_of(const void *h, size_t bytes)
{
    void *d = NULL;
    CHECK(harness_dev_alloc_copy(&d, h, bytes + 16) == 0, "device alloc");
    return d;
}

static void expect_dev(const void *d, const void *exp, size_t bytes, const char *what)
{
    char *got = malloc(bytes + 1);
    CHECK(harness_dev_copy_back(got, d, bytes) == 0, "copy back");
    for (size_t i = 0; i < bytes; ++i)
        CHECK(got[i] == ((const char *) exp)[i], "%s: byte %zu of %zu differs", what, i, bytes);
    free(got);
}

static void wait_free(ompi_request_t **rq, int persistent)
{
    if (persistent) CHECK((*rq)->req_start(1, rq) == OMPI_SUCCESS, "start");
    while (!REQUEST_COMPLETE(*rq)) opal_progress();
    CHECK((*rq)->req_status.MPI_ERROR == OMPI_SUCCESS, "request error %d", (*rq)->req_status.MPI_ERROR);
    if (persistent) (*rq)->req_state = OMPI_REQUEST_INACTIVE;
    CHECK((*rq)->req_free(rq) == OMPI_SUCCESS, "request free");
}

enum { F_BLOCKING, F_NONBLOCKING, F_PERSISTENT };

/* Uniform alltoall of `count` float elements per pair, or — vec — of `count`
 * elements of the gapped type (2 doubles every 4) on the send side received
 * as 2 * count contiguous doubles. */
static void run_alltoall(mca_coll_base_comm_coll_t *t, ompi_communicator_t *comm, int count, int vec,
                         int form, int salt, int expect_saved)
{
    ompi_datatype_t dfloat = {0, 4, 1, 1}, ddouble = {1, 8, 1, 1}, dvec = {1, 16, 1, 0};
    const int n = g_size, me = g_rank;
    const size_t per = vec ? 2 * (size_t) count : (size_t) count;  /* scalars per pair */
    const size_t es = vec ? 8 : 4;
    const size_t sbytes = vec ? (size_t) n * (size_t) count * 32 : (size_t) n * per * es;
    const size_t rbytes = (size_t) n * per * es;
    char *s = malloc(sbytes + 16), *exp = malloc(rbytes + 16);
    void *ds, *dr;
    ompi_request_t *rq = NULL;
    const int before = saved_calls[0];
    int rc;
    memset(s, 0x5A, sbytes + 16);
    for (int q = 0; q < n; ++q) {
        for (size_t i = 0; i < per; ++i) {
            if (vec) {  /* scalar i of the block: element i / 2 of the gapped type, double i % 2 */
                const size_t at = ((size_t) q * (size_t) count + i / 2) * 32 + (i % 2) * 8;
                const double v = val(me, q, i, salt);
                memcpy(s + at, &v, 8);
                const double w = val(q, me, i, salt);
                memcpy(exp + ((size_t) q * per + i) * 8, &w, 8);
            } else {
                ((float *) s)[(size_t) q * per + i] = (float) val(me, q, i, salt);
                ((float *) exp)[(size_t) q * per + i] = (float) val(q, me, i, salt);
            }
        }
    }
    ds = dev_of(s, sbytes);
    {
        char *zero = calloc(1, rbytes + 16);
        dr = dev_of(zero, rbytes);
        free(zero);
    }
    if (F_BLOCKING == form)
        rc = t->coll_alltoall(ds, count, vec ? &dvec : &dfloat, dr, (int) per, vec ? &ddouble : &dfloat,
                              comm, t->coll_alltoall_module);
    else if (F_NONBLOCKING == form)
        rc = t->coll_ialltoall(ds, count, vec ? &dvec : &dfloat, dr, (int) per,
                               vec ? &ddouble : &dfloat, comm, &rq, t->coll_ialltoall_module);
    else
        rc = t->coll_alltoall_init(ds, count, vec ? &dvec : &dfloat, dr, (int) per,
                                   vec ? &ddouble : &dfloat, comm, NULL, &rq,
                                   t->coll_alltoall_init_module);
    CHECK(rc == OMPI_SUCCESS, "alltoall form %d rc %d", form, rc);
    if (F_BLOCKING != form) wait_free(&rq, F_PERSISTENT == form);
    CHECK(saved_calls[0] - before == expect_saved, "alltoall: %d saved calls, expected %d",
          saved_calls[0] - before, expect_saved);
    if (!expect_saved) expect_dev(dr, exp, rbytes, vec ? "alltoall (vector send type)" : "alltoall");
    harness_dev_free(ds);
    harness_dev_free(dr);
    free(s);
    free(exp);
}

/* alltoallv: pair p -> q carries cnt(p, q) elements; the send side is float,
 * or — vec — the gapped type (an element = 2 doubles, extent 4 doubles)
 * received as doubles; the receive side has a 3-scalar gap before every
 * block, which must keep its prefill. */
static int cnt(int p, int q) { return (p + 2 * q) % 3 == 0 ? 0 : 5 + 3 * p + 7 * q; }

static void run_alltoallv(mca_coll_base_comm_coll_t *t, ompi_communicator_t *comm, int vec, int form,
                          int salt)
{
    ompi_datatype_t dfloat = {0, 4, 1, 1}, ddouble = {1, 8, 1, 1}, dvec = {1, 16, 1, 0};
    const int n = g_size, me = g_rank, k = vec ? 2 : 1;  /* scalars per send element */
    const size_t es = vec ? 8 : 4, sext = vec ? 32 : 4;
    int sc[OMPI_AMD_MAX_RANKS], sd[OMPI_AMD_MAX_RANKS], rc_[OMPI_AMD_MAX_RANKS], rd[OMPI_AMD_MAX_RANKS];
    int sat = 1, rat = 0, rc;
    for (int q = n - 1; q >= 0; --q) {  /* send blocks in descending order, one element apart */
        sc[q] = cnt(me, q);
        sd[q] = sat;
        sat += sc[q] + 1;
    }
    for (int p = 0; p < n; ++p) {
        rc_[p] = k * cnt(p, me);
        rd[p] = rat + 3;
        rat = rd[p] + rc_[p];
    }
    const size_t sbytes = (size_t) sat * sext, rbytes = (size_t) (rat + 3) * es;
    char *s = malloc(sbytes + 16), *exp = malloc(rbytes + 16);
    void *ds, *dr;
    ompi_request_t *rq = NULL;
    const int before = saved_calls[1];
    memset(s, 0x5A, sbytes + 16);
    memset(exp, 0x5A, rbytes + 16);
    for (int q = 0; q < n; ++q) {
        for (size_t i = 0; i < (size_t) (k * sc[q]); ++i) {
            if (vec) {
                const double v = val(me, q, i, salt);
                memcpy(s + ((size_t) sd[q] + i / 2) * 32 + (i % 2) * 8, &v, 8);
            } else {
                ((float *) s)[(size_t) sd[q] + i] = (float) val(me, q, i, salt);
            }
        }
        for (size_t i = 0; i < (size_t) rc_[q]; ++i) {
            if (vec) {
                const double w = val(q, me, i, salt);
                memcpy(exp + ((size_t) rd[q] + i) * 8, &w, 8);
            } else {
                ((float *) exp)[(size_t) rd[q] + i] = (float) val(q, me, i, salt);
            }
        }
    }
    ds = dev_of(s, sbytes);
    {
        char *pre = malloc(rbytes + 16);
        memset(pre, 0x5A, rbytes + 16);
        dr = dev_of(pre, rbytes);
        free(pre);
    }
    if (F_BLOCKING == form)
        rc = t->coll_alltoallv(ds, sc, sd, vec ? &dvec : &dfloat, dr, rc_, rd, vec ? &ddouble : &dfloat,
                               comm, t->coll_alltoallv_module);
    else if (F_NONBLOCKING == form)
        rc = t->coll_ialltoallv(ds, sc, sd, vec ? &dvec : &dfloat, dr, rc_, rd,
                                vec ? &ddouble : &dfloat, comm, &rq, t->coll_ialltoallv_module);
    else
        rc = t->coll_alltoallv_init(ds, sc, sd, vec ? &dvec : &dfloat, dr, rc_, rd,
                                    vec ? &ddouble : &dfloat, comm, NULL, &rq,
                                    t->coll_alltoallv_init_module);
    CHECK(rc == OMPI_SUCCESS, "alltoallv form %d rc %d", form, rc);
    if (F_BLOCKING != form) wait_free(&rq, F_PERSISTENT == form);
    CHECK(saved_calls[1] == before, "alltoallv on device buffers reached the saved function");
    expect_dev(dr, exp, rbytes, vec ? "alltoallv (vector send type)" : "alltoallv");
    harness_dev_free(ds);
    harness_dev_free(dr);
    free(s);
    free(exp);
}

int main(int argc, char **argv)
{
    const int use_gpu = getenv("HARNESS_GPU") && atoi(getenv("HARNESS_GPU"));
    ompi_group_t local = {0};
    mca_coll_base_comm_coll_t table;
    ompi_communicator_t comm;
    mca_coll_base_module_t *tm, *m;
    ompi_datatype_t dfloat = {0, 4, 1, 1};
    int prio = -1, refs;

    if (argc < 4) return 2;
    g_rank = atoi(argv[2]);
    g_size = atoi(argv[3]);
    harness_proc_name.jobid = (unsigned) strtoul(argv[1], NULL, 16);
    for (int i = 0; i < 64; ++i) ompi_op_ddt_map[i] = i;

    tm = OBJ_NEW(mca_coll_base_module_t);
    memset(&table, 0, sizeof(table));
#define FILL(fn) table.coll_##fn##_module = tm; OBJ_RETAIN(tm);
    OTHER_SLOTS(FILL)
    A2A_SLOTS(FILL)
#undef FILL
    table.coll_alltoall = sv_alltoall;
    table.coll_alltoallv = sv_alltoallv;
    table.coll_ialltoall = sv_ialltoall;
    table.coll_ialltoallv = sv_ialltoallv;
    table.coll_alltoall_init = sv_alltoall_init;
    table.coll_alltoallv_init = sv_alltoallv_init;
    comm = (ompi_communicator_t){g_rank, g_size, 5, 0, &local, &table};
    refs = tm->super.obj_reference_count;

    m = mca_coll_rocm_component.super.collm_comm_query(&comm, &prio);
    CHECK(m != NULL, "comm_query");
    CHECK(m->coll_alltoall && m->coll_alltoallv && m->coll_ialltoall && m->coll_ialltoallv &&
              m->coll_alltoall_init && m->coll_alltoallv_init, "the six alltoall slots");
    if (!use_gpu) {
        OBJ_RELEASE(m);
        printf("ok\n");
        return 0;
    }

    mca_coll_rocm_component.residency_lock = 0;  /* the per-call vote, never locks */
    CHECK(m->coll_module_enable(m, &comm) == OMPI_SUCCESS, "enable");
    CHECK(tm->super.obj_reference_count == refs + 30, "enable retains 30 saved modules (%d)",
          tm->super.obj_reference_count - refs);
#define INST(fn) OBJ_RELEASE(table.coll_##fn##_module); table.coll_##fn = m->coll_##fn; \
                 table.coll_##fn##_module = m; OBJ_RETAIN(m);
    A2A_SLOTS(INST)
#undef INST

    /* 1. device buffers: the device path, exact, no saved call */
    run_alltoall(&table, &comm, 300, 0, F_BLOCKING, 1, 0);
    run_alltoall(&table, &comm, 300001, 0, F_BLOCKING, 2, 0);  /* 1.2 MB per pair: the landing path */
    run_alltoall(&table, &comm, 300, 0, F_NONBLOCKING, 3, 0);
    run_alltoall(&table, &comm, 300, 0, F_PERSISTENT, 4, 0);
    run_alltoallv(&table, &comm, 0, F_BLOCKING, 5);
    run_alltoallv(&table, &comm, 0, F_NONBLOCKING, 6);  /* completes through the request */
    run_alltoallv(&table, &comm, 0, F_PERSISTENT, 7);

    /* 2. host buffers reach the saved function, as host pointers */
    {
        const size_t b = (size_t) g_size * 64 * sizeof(float);
        float *hs = calloc(1, b), *hr = calloc(1, b);
        int c[OMPI_AMD_MAX_RANKS], d[OMPI_AMD_MAX_RANKS];
        for (int p = 0; p < g_size; ++p) { c[p] = 64; d[p] = 64 * p; }
        CHECK(table.coll_alltoall(hs, 64, &dfloat, hr, 64, &dfloat, &comm, table.coll_alltoall_module) ==
                  OMPI_SUCCESS && saved_calls[0] == 1, "host alltoall -> saved (%d)", saved_calls[0]);
        CHECK(table.coll_alltoallv(hs, c, d, &dfloat, hr, c, d, &dfloat, &comm,
                                   table.coll_alltoallv_module) == OMPI_SUCCESS && saved_calls[1] == 1,
              "host alltoallv -> saved (%d)", saved_calls[1]);
        CHECK(saved_dev == 0, "a saved function saw a device pointer");
        free(hs);
        free(hr);
    }

    /* 3. a blocking alltoall whose send and receive byte counts differ is
     * declined to the saved function (with host copies of the device operands) */
    {
        ompi_datatype_t ddouble = {1, 8, 1, 1};
        const size_t b = (size_t) g_size * 32 * 8;
        char *z = calloc(1, b + 16);
        void *ds = dev_of(z, b), *dr = dev_of(z, b);
        CHECK(table.coll_alltoall(ds, 32, &dfloat, dr, 32, &ddouble, &comm, table.coll_alltoall_module) ==
                  OMPI_SUCCESS && saved_calls[0] == 2, "unequal byte counts -> saved (%d)", saved_calls[0]);
        CHECK(saved_dev == 0, "the declined call handed device memory to the saved function");
        harness_dev_free(ds);
        harness_dev_free(dr);
        free(z);
    }

    /* 4. under the DEVICE lock (one unanimous device call locks it) a
     * vector-typed send operand is packed: 2 doubles every 4 */
    mca_coll_rocm_component.residency_lock = 1;
    run_alltoall(&table, &comm, 300, 0, F_BLOCKING, 8, 0);
    CHECK(((mca_coll_rocm_module_t *) m)->mode == ROCM_RES_DEVICE, "locked to DEVICE");
    run_alltoall(&table, &comm, 37, 1, F_BLOCKING, 9, 0);
    run_alltoall(&table, &comm, 37, 1, F_NONBLOCKING, 10, 0);
    run_alltoallv(&table, &comm, 1, F_BLOCKING, 11);
    run_alltoallv(&table, &comm, 1, F_NONBLOCKING, 12);
    run_alltoallv(&table, &comm, 1, F_PERSISTENT, 13);

    /* 5. release: the module drops what enable retained */
#define UNINST(fn) OBJ_RELEASE(table.coll_##fn##_module); table.coll_##fn##_module = NULL;
    A2A_SLOTS(UNINST)
#undef UNINST
    OBJ_RELEASE(m);
    CHECK(tm->super.obj_reference_count == refs - 6, "release (%d, expected %d)",
          tm->super.obj_reference_count, refs - 6);
    printf("ok gpu\n");
    return 0;
}
