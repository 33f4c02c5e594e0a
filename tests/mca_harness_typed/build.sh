#!/bin/bash
# TEST HARNESS ONLY: compile ompi_amd/mca/coll/rocm with ROCM_HAVE_TYPED_XCH
# (and both groups of exchange slots) against the stand-in coll.h and
# ompi_datatype.h of this directory (placed before the stand-ins of
# tests/mca_harness, which supply everything else) and link libompi_amd.
#   build.sh OUT          the harness binary
#   build.sh --syntax     only compile the glue, warnings are errors
#   build.sh --syntax-without   the glue alone without ROCM_HAVE_TYPED_XCH
set -e
H=$(cd "$(dirname "$0")" && pwd)
R=$(cd "$H/../.." && pwd)
O=$R/tests/mca_harness
FLAGS="-std=gnu11 -O1 -DHARNESS_COLL -DHARNESS_COLL_ALLTOALL -DHARNESS_COLL_GATHER -DROCM_HAVE_TYPED_XCH -Wall -Wextra -Wno-unused-parameter -Wno-missing-field-initializers"
INC="-I$H/coll_include -I$O/coll_include -I$O/include -I$R/include -I$R/ompi_amd/mca/coll/rocm -I/opt/rocm/include"
if [ "$1" = "--syntax-without" ]; then  # the same glue, same headers, macro off
    exec gcc ${FLAGS/-DROCM_HAVE_TYPED_XCH/} -Werror -fsyntax-only $INC "$R/ompi_amd/mca/coll/rocm/coll_rocm_module.c"
fi
if [ "$1" = "--syntax" ]; then
    exec gcc $FLAGS -Werror -fsyntax-only $INC "$R/ompi_amd/mca/coll/rocm/coll_rocm_module.c" "$H/typed_harness.c"
fi
OUT=${1:-$H/typed_harness}
gcc $FLAGS $INC \
    "$R/ompi_amd/mca/coll/rocm/coll_rocm_module.c" "$H/typed_harness.c" "$O/dev_helpers.c" "$O/progress_stub.c" \
    -L"$R/ompi_amd" -lompi_amd -L/opt/rocm/lib -lamdhip64 \
    -Wl,-rpath,"$R/ompi_amd" -Wl,-rpath,/opt/rocm/lib -lrt -o "$OUT"
