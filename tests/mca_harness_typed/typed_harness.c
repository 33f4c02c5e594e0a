/*
 * TEST HARNESS ONLY.  One rank of a multi-process run that drives the
 * twenty-one exchange slots of ompi_amd/mca/coll/rocm/coll_rocm_module.c
 * (alltoall, alltoallv, allgatherv, gather, gatherv, scatter, scatterv, each
 * blocking, nonblocking and persistent) built with ROCM_HAVE_TYPED_XCH, the
 * way the coll framework does: recording stand-ins are the previously
 * selected functions, the module is enabled under coll_rocm_residency = device
 * (a non-contiguous operand reaches the device path only there: the vote is
 * on contiguous device operands, with or without the macro) and its functions
 * are installed in the communicator's table.
 *
 *   CPU (HARNESS_GPU=0): the module offers the twenty-one slots.
 *   GPU (HARNESS_GPU=1): device operands of the gapped stand-in type (`size`
 *   data bytes, then a `size`-byte gap) on the send side, the receive side,
 *   both, and on the odd ranks only (the others pass the contiguous type of
 *   the same signature): exact results, every gap and every byte between
 *   blocks keeps its prefill, the saved function is not called, and the
 *   module's typed_calls counter moves exactly when this rank has a
 *   significant gapped operand; in place at the root / on every rank; a
 *   gapped type WITHOUT a device program still takes the packed path, exact,
 *   and the counter stands still.
 *
 * usage: typed_harness <segment-name> <rank> <size>; prints "ok" / "ok gpu".
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
#include "ompi_amd_ddt.h"

extern mca_coll_rocm_component_t mca_coll_rocm_component;
extern int harness_dev_alloc_copy(void **d, const void *h, size_t bytes);
extern int harness_dev_copy_back(void *h, const void *d, size_t bytes);
extern int harness_dev_free(void *d);

OBJ_CLASS_INSTANCE(mca_coll_base_module_t, opal_object_t, NULL, NULL);
harness_proc_name_t harness_proc_name = {4245, 0};
int ompi_op_ddt_map[64];
struct ompi_datatype_t harness_mpi_byte = {2, 1, 1, 1, 0};

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

/* common/rocm's device program of a datatype (opal_datatype_rocm.c) for the
 * stand-in types: one run of `size` bytes, extent 2 * `size` when gapped;
 * NULL for a type marked no_program */
struct opal_datatype_t;
static int device_ddt_lookups;
const ompi_amd_ddt_t *opal_rocm_device_ddt(const struct opal_datatype_t *dt)
{
    static struct { size_t size; int contiguous; ompi_amd_ddt_t *prog; } cache[16];
    static int n;
    const ompi_datatype_t *d = (const ompi_datatype_t *) dt;
    ompi_amd_ddt_elem_t e = {1, (int64_t) d->size, (int64_t) d->size, 0};
    ompi_amd_ddt_t *prog = NULL;
    ++device_ddt_lookups;
    if (d->no_program) return NULL;
    for (int i = 0; i < n; ++i)
        if (cache[i].size == d->size && cache[i].contiguous == d->contiguous) return cache[i].prog;
    if (16 == n || ompi_amd_ddt_create_elems(&e, 1, (int64_t) (d->contiguous ? d->size : 2 * d->size),
                                             &prog) != 0)
        return NULL;
    cache[n].size = d->size;
    cache[n].contiguous = d->contiguous;
    cache[n++].prog = prog;
    return prog;
}

enum { K_ALLTOALL, K_ALLTOALLV, K_ALLGATHERV, K_GATHER, K_GATHERV, K_SCATTER, K_SCATTERV, K_COUNT };
enum { F_BLOCKING, F_NONBLOCKING, F_PERSISTENT };
/* which operands are the gapped type */
enum { V_SEND, V_RECV, V_BOTH, V_ODD_RANKS, V_NO_PROGRAM, V_COUNT };
static const char *kname[K_COUNT] = {"alltoall", "alltoallv", "allgatherv", "gather",
                                     "gatherv", "scatter", "scatterv"};

/* ---- the recording saved functions ---- */
static int saved_calls;
#define A2A_P const void *s, int sc, struct ompi_datatype_t *sd, void *r, int rc, struct ompi_datatype_t *rd
#define A2AV_P const void *s, const int *sc, const int *sp, struct ompi_datatype_t *sd, void *r, const int *rc, const int *rp, struct ompi_datatype_t *rd
#define AGV_P const void *s, int sc, struct ompi_datatype_t *sd, void *r, const int *rc, const int *dp, struct ompi_datatype_t *rd
#define ROOTED_P A2A_P, int root
#define GATHERV_P AGV_P, int root
#define SCATTERV_P const void *s, const int *sc, const int *dp, struct ompi_datatype_t *sd, void *r, int rc, struct ompi_datatype_t *rd, int root
#define SAVED3(name, P)                                                                        \
    static int sv_##name(P, struct ompi_communicator_t *c, mca_coll_base_module_t *m)          \
    {                                                                                          \
        ++saved_calls;                                                                         \
        return OMPI_SUCCESS;                                                                   \
    }                                                                                          \
    static int sv_i##name(P, struct ompi_communicator_t *c, ompi_request_t **rq,               \
                          mca_coll_base_module_t *m)                                           \
    {                                                                                          \
        ++saved_calls;                                                                         \
        return OMPI_ERROR;                                                                     \
    }                                                                                          \
    static int sv_##name##_init(P, struct ompi_communicator_t *c, struct ompi_info_t *info,    \
                                ompi_request_t **rq, mca_coll_base_module_t *m)                \
    {                                                                                          \
        ++saved_calls;                                                                         \
        return OMPI_ERROR;                                                                     \
    }
SAVED3(alltoall, A2A_P)
SAVED3(alltoallv, A2AV_P)
SAVED3(allgatherv, AGV_P)
SAVED3(gather, ROOTED_P)
SAVED3(gatherv, GATHERV_P)
SAVED3(scatter, ROOTED_P)
SAVED3(scatterv, SCATTERV_P)

/* byte i of the block rank p sends to rank q */
static unsigned char val(int p, int q, size_t i, int salt)
{
    return (unsigned char) (p * 131 + q * 29 + (int) (i * 7) + (int) (i >> 8) * 13 + salt * 17 + 3);
}

/* A buffer of `elems` elements of `es` bytes: the logical image (contiguous,
 * prefilled with 0x5A) and its place on the device in the operand's layout
 * (gapped: element e at 2 * es * e, the gaps and 16 trailing bytes 0x5A). */
typedef struct {
    size_t elems, es;
    int gapped;
    char *logical;
    void *dev;
} buf_t;

static size_t phys_bytes(const buf_t *b) { return b->elems * b->es * (b->gapped ? 2 : 1) + 16; }

static char *expand(const buf_t *b, const char *logical)
{
    const size_t ext = b->es * (b->gapped ? 2 : 1);
    char *p = malloc(phys_bytes(b));
    memset(p, 0x5A, phys_bytes(b));
    for (size_t e = 0; e < b->elems; ++e) memcpy(p + e * ext, logical + e * b->es, b->es);
    return p;
}

static void buf_init(buf_t *b, size_t elems, size_t es, int gapped)
{
    b->elems = elems;
    b->es = es;
    b->gapped = gapped;
    b->logical = malloc(elems * es + 1);
    memset(b->logical, 0x5A, elems * es + 1);
    b->dev = NULL;
}

static void buf_upload(buf_t *b)
{
    char *p = expand(b, b->logical);
    CHECK(harness_dev_alloc_copy(&b->dev, p, phys_bytes(b)) == 0, "device alloc");
    free(p);
}

/* the device image is exactly the layout of `logical`: data, gaps, trailer */
static void buf_expect(const buf_t *b, const char *logical, const char *what)
{
    char *exp = expand(b, logical), *got = malloc(phys_bytes(b));
    CHECK(harness_dev_copy_back(got, b->dev, phys_bytes(b)) == 0, "copy back");
    for (size_t i = 0; i < phys_bytes(b); ++i)
        CHECK(got[i] == exp[i], "%s: byte %zu of %zu differs (got %02x, expected %02x)", what, i,
              phys_bytes(b), (unsigned char) got[i], (unsigned char) exp[i]);
    free(exp);
    free(got);
}

static void buf_free(buf_t *b)
{
    if (b->dev) harness_dev_free(b->dev);
    free(b->logical);
}

static void wait_free(ompi_request_t **rq, int persistent)
{
    if (persistent) CHECK((*rq)->req_start(1, rq) == OMPI_SUCCESS, "start");
    while (!REQUEST_COMPLETE(*rq)) opal_progress();
    CHECK((*rq)->req_status.MPI_ERROR == OMPI_SUCCESS, "request error %d", (*rq)->req_status.MPI_ERROR);
    if (persistent) (*rq)->req_state = OMPI_REQUEST_INACTIVE;
    CHECK((*rq)->req_free(rq) == OMPI_SUCCESS, "request free");
}

/* elements in the block p sends to q */
static int pair_count(int kind, int p, int q)
{
    switch (kind) {
    case K_ALLTOALLV: return (p + 2 * q) % 3 == 0 ? 0 : 5 + 3 * p + 2 * q;
    case K_ALLGATHERV:
    case K_GATHERV: return 5 + 3 * p;
    case K_SCATTERV: return 5 + 3 * q;
    default: return 7;
    }
}

/* One call of `kind` in `form` on device buffers of `es`-byte elements with
 * the gapped type where `variant` says.  Vector kinds leave a one-element gap
 * before every block of an n-block operand.  Expected bytes come from val(). */
static void run(mca_coll_base_comm_coll_t *t, ompi_communicator_t *comm, mca_coll_rocm_module_t *mod,
                int kind, int form, int variant, size_t es, int root, int inplace, int salt)
{
    const int n = g_size, me = g_rank;
    const int vec = K_ALLTOALLV == kind || K_ALLGATHERV == kind || K_GATHERV == kind || K_SCATTERV == kind;
    const int rooted = kind >= K_GATHER, scatter = K_SCATTER == kind || K_SCATTERV == kind;
    const int is_root = !rooted || me == root;
    const int a2a = K_ALLTOALL == kind || K_ALLTOALLV == kind;
    /* the side with n blocks here, the side with one block */
    const int s_wide = a2a || (scatter && is_root), r_wide = a2a || K_ALLGATHERV == kind || (!scatter && rooted && is_root);
    const int s_here = !rooted || !scatter || is_root, r_here = !rooted || scatter || is_root;
    const int odd = V_ODD_RANKS == variant;
    const int s_gap = odd ? me % 2 : (V_RECV != variant), r_gap = odd ? 0 : (V_SEND != variant);
    ompi_datatype_t sdt = {es == 4 ? 0 : 3, es, 1, !s_gap, V_NO_PROGRAM == variant};
    ompi_datatype_t rdt = {es == 4 ? 0 : 3, es, 1, !r_gap, V_NO_PROGRAM == variant};
    int sc[OMPI_AMD_MAX_RANKS], sd[OMPI_AMD_MAX_RANKS], rc_[OMPI_AMD_MAX_RANKS], rd[OMPI_AMD_MAX_RANKS];
    int sat = 0, rat = 0, rc, expect_typed;
    const int before = saved_calls, typed_before = mod->typed_calls;
    ompi_request_t *rq = NULL;
    buf_t sb, rb;
    char *exp, what[128];

    if (K_ALLTOALLV == kind) inplace = 0;  /* its counts are not symmetric */
    /* in place: every rank (alltoall, allgatherv) or the root */
    inplace = inplace && (a2a || K_ALLGATHERV == kind || (rooted && me == root));
    snprintf(what, sizeof(what), "%s form %d variant %d es %zu root %d inplace %d", kname[kind], form,
             variant, es, root, inplace);
    for (int p = 0; p < n; ++p) {
        /* what I send to p, what p sends to me; scatter's / gather's sender
         * or receiver is the root */
        sc[p] = s_wide ? pair_count(kind, me, p) : 0;
        sd[p] = sat + (vec ? 1 : 0);
        sat = sd[p] + sc[p];
        rc_[p] = r_wide ? pair_count(kind, p, me) : 0;
        rd[p] = rat + (vec ? 1 : 0);
        rat = rd[p] + rc_[p];
    }
    /* the one-block sides */
    const int s_one = pair_count(kind, me, rooted ? root : me), r_one = pair_count(kind, root, me);
    if (!s_wide) sat = s_one;
    if (!r_wide) rat = r_one;
    buf_init(&sb, s_here ? (size_t) sat + (s_wide && vec) : 0, es, s_gap);
    buf_init(&rb, r_here ? (size_t) rat + (r_wide && vec) : 0, es, r_gap);
    exp = malloc(rb.elems * es + 1);
    memset(exp, 0x5A, rb.elems * es + 1);

    /* the send image, and what the receive image must become */
    if (s_here && s_wide)
        for (int q = 0; q < n; ++q)
            for (size_t i = 0; i < (size_t) sc[q] * es; ++i) sb.logical[(size_t) sd[q] * es + i] = (char) val(me, q, i, salt);
    if (s_here && !s_wide)  /* allgatherv / gather(v): my block, the same for every receiver */
        for (size_t i = 0; i < (size_t) s_one * es; ++i) sb.logical[i] = (char) val(me, -1, i, salt);
    if (r_here && r_wide)
        for (int p = 0; p < n; ++p)
            for (size_t i = 0; i < (size_t) rc_[p] * es; ++i)
                exp[(size_t) rd[p] * es + i] = (char) val(p, a2a ? me : -1, i, salt);
    if (r_here && !r_wide)  /* scatter(v): my block of the root's operand */
        for (size_t i = 0; i < (size_t) r_one * es; ++i) exp[i] = (char) val(root, me, i, salt);
    if (inplace && !scatter) {  /* my contribution already sits in the receive operand */
        if (a2a)
            for (int q = 0; q < n; ++q)
                for (size_t i = 0; i < (size_t) rc_[q] * es; ++i) rb.logical[(size_t) rd[q] * es + i] = (char) val(me, q, i, salt);
        else
            for (size_t i = 0; i < (size_t) rc_[me] * es; ++i) rb.logical[(size_t) rd[me] * es + i] = (char) val(me, -1, i, salt);
    }
    if (s_here && !(inplace && !scatter)) buf_upload(&sb);
    if (r_here && !(inplace && scatter)) buf_upload(&rb);
    {
        const void *s = inplace && !scatter ? MPI_IN_PLACE : sb.dev;
        void *r = inplace && scatter ? MPI_IN_PLACE : rb.dev;
        const int *scs = s_wide ? sc : NULL, *sds = s_wide ? sd : NULL;
        const int *rcs = r_wide ? rc_ : NULL, *rds = r_wide ? rd : NULL;
#define CALL3(X, ...)                                                                          \
    (F_BLOCKING == form      ? t->coll_##X(__VA_ARGS__, comm, t->coll_##X##_module)            \
     : F_NONBLOCKING == form ? t->coll_i##X(__VA_ARGS__, comm, &rq, t->coll_i##X##_module)     \
                             : t->coll_##X##_init(__VA_ARGS__, comm, NULL, &rq, t->coll_##X##_init_module))
        switch (kind) {
        case K_ALLTOALL: rc = CALL3(alltoall, s, 7, &sdt, r, 7, &rdt); break;
        case K_ALLTOALLV: rc = CALL3(alltoallv, s, sc, sd, &sdt, r, rc_, rd, &rdt); break;
        case K_ALLGATHERV: rc = CALL3(allgatherv, s, s_one, &sdt, r, rc_, rd, &rdt); break;
        case K_GATHER: rc = CALL3(gather, s, 7, &sdt, r, 7, &rdt, root); break;
        case K_GATHERV: rc = CALL3(gatherv, s, s_one, &sdt, r, rcs, rds, &rdt, root); break;
        case K_SCATTER: rc = CALL3(scatter, s, 7, &sdt, r, 7, &rdt, root); break;
        default: rc = CALL3(scatterv, s, scs, sds, &sdt, r, r_one, &rdt, root); break;
        }
#undef CALL3
    }
    CHECK(rc == OMPI_SUCCESS, "%s: rc %d", what, rc);
    if (F_BLOCKING != form) wait_free(&rq, F_PERSISTENT == form);
    CHECK(saved_calls == before, "%s: device buffers reached the saved function", what);
    if (rb.dev) buf_expect(&rb, exp, what);
    if (sb.dev) buf_expect(&sb, sb.logical, what);  /* the source is unchanged */
    /* the typed path: this rank has a gapped device operand with a program */
    expect_typed = V_NO_PROGRAM != variant && ((sb.dev && s_gap && sb.elems) || (rb.dev && r_gap && rb.elems));
    CHECK(mod->typed_calls - typed_before == expect_typed, "%s: typed_calls moved by %d, expected %d", what,
          mod->typed_calls - typed_before, expect_typed);
    buf_free(&sb);
    buf_free(&rb);
    free(exp);
}

int main(int argc, char **argv)
{
    const int use_gpu = getenv("HARNESS_GPU") && atoi(getenv("HARNESS_GPU"));
    ompi_group_t local = {0};
    mca_coll_base_comm_coll_t table;
    ompi_communicator_t comm;
    mca_coll_base_module_t *tm, *m;
    int prio = -1, salt = 0;

    if (argc < 4) return 2;
    g_rank = atoi(argv[2]);
    g_size = atoi(argv[3]);
    harness_proc_name.jobid = (unsigned) strtoul(argv[1], NULL, 16);
    for (int i = 0; i < 64; ++i) ompi_op_ddt_map[i] = i;

    tm = OBJ_NEW(mca_coll_base_module_t);
    memset(&table, 0, sizeof(table));
#define FILL(fn) table.coll_##fn##_module = tm; OBJ_RETAIN(tm);
    H_ALL_SLOTS(FILL)
#undef FILL
#define STANDIN(fn) table.coll_##fn = sv_##fn;
    H_XCH_SLOTS(STANDIN)
#undef STANDIN
    comm = (ompi_communicator_t){g_rank, g_size, 7, 0, &local, &table};

    m = mca_coll_rocm_component.super.collm_comm_query(&comm, &prio);
    CHECK(m != NULL, "comm_query");
#define OFFERED(fn) CHECK(m->coll_##fn != NULL, "slot " #fn " not offered");
    H_XCH_SLOTS(OFFERED)
#undef OFFERED
    if (!use_gpu) {
        OBJ_RELEASE(m);
        printf("ok\n");
        return 0;
    }

    mca_coll_rocm_component.residency = ROCM_RES_DEVICE;
    CHECK(m->coll_module_enable(m, &comm) == OMPI_SUCCESS, "enable");
#define INST(fn) OBJ_RELEASE(table.coll_##fn##_module); table.coll_##fn = m->coll_##fn; \
                 table.coll_##fn##_module = m; OBJ_RETAIN(m);
    H_XCH_SLOTS(INST)
#undef INST

    /* every collective, form and variant (the no-program fallback among
     * them), 4- and 16-byte elements alternating, the root moving; then in
     * place with both sides gapped */
    for (int kind = 0; kind < K_COUNT; ++kind)
        for (int form = F_BLOCKING; form <= F_PERSISTENT; ++form) {
            for (int variant = 0; variant < V_COUNT; ++variant)
                run(&table, &comm, (mca_coll_rocm_module_t *) m, kind, form, variant,
                    (kind + form + variant) % 2 ? 16 : 4, (kind + form + variant) % g_size, 0, ++salt);
            run(&table, &comm, (mca_coll_rocm_module_t *) m, kind, form, V_BOTH, 4, (kind + form) % g_size, 1,
                ++salt);
        }
    CHECK(device_ddt_lookups > 0, "opal_rocm_device_ddt was never asked");

#define UNINST(fn) OBJ_RELEASE(table.coll_##fn##_module); table.coll_##fn##_module = NULL;
    H_XCH_SLOTS(UNINST)
#undef UNINST
    OBJ_RELEASE(m);
    printf("ok gpu\n");
    return 0;
}
