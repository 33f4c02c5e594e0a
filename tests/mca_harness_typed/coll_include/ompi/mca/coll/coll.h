/* TEST HARNESS ONLY: a stand-in for ompi/mca/coll/coll.h with every slot
 * coll/rocm saves and offers in a HARNESS_COLL + HARNESS_COLL_ALLTOALL +
 * HARNESS_COLL_GATHER build: the twenty-four of tests/mca_harness/coll_include,
 * the fifteen of allgatherv / gather / gatherv / scatter / scatterv and the
 * six of alltoall / alltoallv (blocking, nonblocking, persistent).  It restates the slot signatures (operands; root where there
 * is one; communicator; info for the persistent form; request for the
 * nonblocking and persistent forms; module) and the field order the
 * component needs.  The typed-exchange harness puts this
 * directory first on the include path; the include guard is the other
 * stand-in's, so only one of them is seen. */
#ifndef HARNESS_COLL_H
#define HARNESS_COLL_H
#include <stdbool.h>
#include "ompi/mca/mca.h"
#include "opal/class/opal_object.h"
#include "ompi/request/request.h"
struct ompi_communicator_t;
struct ompi_info_t;
struct ompi_datatype_t;
struct ompi_op_t;
struct mca_coll_base_module_2_3_0_t;

/* operand lists */
#define H_DT struct ompi_datatype_t *
#define H_REDUCE const void *, void *, int, H_DT, struct ompi_op_t *
#define H_REDUCE_ROOT H_REDUCE, int
#define H_REDUCE_V const void *, void *, const int *, H_DT, struct ompi_op_t *
#define H_ALLGATHER const void *, int, H_DT, void *, int, H_DT
#define H_BCAST void *, int, H_DT, int
#define H_ALLGATHERV const void *, int, H_DT, void *, const int *, const int *, H_DT
#define H_ROOTED H_ALLGATHER, int
#define H_GATHERV H_ALLGATHERV, int
#define H_SCATTERV const void *, const int *, const int *, H_DT, void *, int, H_DT, int
#define H_ALLTOALLV const void *, const int *, const int *, H_DT, void *, const int *, const int *, H_DT
/* the three forms of a slot with operand list ARGS */
#define H_SLOT(name, ARGS)                                                                     \
    typedef int (*mca_coll_base_module_##name##_fn_t)(ARGS, struct ompi_communicator_t *,      \
                                                      struct mca_coll_base_module_2_3_0_t *);  \
    typedef int (*mca_coll_base_module_i##name##_fn_t)(ARGS, struct ompi_communicator_t *,     \
                                                       ompi_request_t **,                      \
                                                       struct mca_coll_base_module_2_3_0_t *); \
    typedef int (*mca_coll_base_module_##name##_init_fn_t)(                                    \
        ARGS, struct ompi_communicator_t *, struct ompi_info_t *, ompi_request_t **,           \
        struct mca_coll_base_module_2_3_0_t *);
H_SLOT(allgather, H_ALLGATHER)
H_SLOT(allreduce, H_REDUCE)
H_SLOT(bcast, H_BCAST)
H_SLOT(exscan, H_REDUCE)
H_SLOT(reduce, H_REDUCE_ROOT)
H_SLOT(reduce_scatter, H_REDUCE_V)
H_SLOT(reduce_scatter_block, H_REDUCE)
H_SLOT(scan, H_REDUCE)
H_SLOT(allgatherv, H_ALLGATHERV)
H_SLOT(gather, H_ROOTED)
H_SLOT(gatherv, H_GATHERV)
H_SLOT(scatter, H_ROOTED)
H_SLOT(scatterv, H_SCATTERV)
H_SLOT(alltoall, H_ALLGATHER)
H_SLOT(alltoallv, H_ALLTOALLV)
typedef int (*mca_coll_base_module_enable_1_1_0_fn_t)(struct mca_coll_base_module_2_3_0_t *,
                                                      struct ompi_communicator_t *);

/* every slot, in the module's field order: X(name) */
#define H_BLOCKING_SLOTS(X)                                                                    \
    X(allgather) X(allreduce) X(bcast) X(exscan) X(reduce) X(reduce_scatter)                   \
    X(reduce_scatter_block) X(scan)
#define H_NONBLOCKING_SLOTS(X)                                                                 \
    X(iallgather) X(iallreduce) X(ibcast) X(ireduce_scatter_block) X(iexscan) X(ireduce)       \
    X(ireduce_scatter) X(iscan)
#define H_PERSISTENT_SLOTS(X)                                                                  \
    X(allgather_init) X(allreduce_init) X(bcast_init) X(reduce_scatter_block_init)             \
    X(exscan_init) X(reduce_init) X(reduce_scatter_init) X(scan_init)
#define H_GATHER_SLOTS(X)                                                                      \
    X(allgatherv) X(gather) X(gatherv) X(scatter) X(scatterv)                                  \
    X(iallgatherv) X(igather) X(igatherv) X(iscatter) X(iscatterv)                             \
    X(allgatherv_init) X(gather_init) X(gatherv_init) X(scatter_init) X(scatterv_init)
#define H_A2A_SLOTS(X)                                                                         \
    X(alltoall) X(alltoallv) X(ialltoall) X(ialltoallv) X(alltoall_init) X(alltoallv_init)
#define H_XCH_SLOTS(X) H_GATHER_SLOTS(X) H_A2A_SLOTS(X)
#define H_ALL_SLOTS(X) H_BLOCKING_SLOTS(X) H_NONBLOCKING_SLOTS(X) H_PERSISTENT_SLOTS(X) H_XCH_SLOTS(X)

#define H_FIELD(name) mca_coll_base_module_##name##_fn_t coll_##name;
typedef struct mca_coll_base_module_2_3_0_t {
    opal_object_t super;
    mca_coll_base_module_enable_1_1_0_fn_t coll_module_enable;
    H_ALL_SLOTS(H_FIELD)
    void *base_data;
} mca_coll_base_module_2_3_0_t;
#undef H_FIELD
typedef mca_coll_base_module_2_3_0_t mca_coll_base_module_t;
OBJ_CLASS_DECLARATION(mca_coll_base_module_t);
typedef int (*mca_coll_base_component_init_query_fn_t)(bool, bool);
typedef mca_coll_base_module_t *(*mca_coll_base_component_comm_query_2_0_0_fn_t)(
    struct ompi_communicator_t *, int *);
typedef struct mca_coll_base_component_2_0_0_t {
    mca_base_component_t collm_version;
    mca_base_component_data_t collm_data;
    mca_coll_base_component_init_query_fn_t collm_init_query;
    mca_coll_base_component_comm_query_2_0_0_fn_t collm_comm_query;
} mca_coll_base_component_2_0_0_t;
/* per-communicator function table: every slot with the module that provides it */
#define H_ENTRY(name) mca_coll_base_module_##name##_fn_t coll_##name; mca_coll_base_module_t *coll_##name##_module;
typedef struct mca_coll_base_comm_coll_t {
    H_ALL_SLOTS(H_ENTRY)
} mca_coll_base_comm_coll_t;
#undef H_ENTRY
#define MCA_COLL_BASE_VERSION_2_0_0 OMPI_MCA_BASE_VERSION_2_1_0("coll", 2, 0, 0)
#endif
