// hode_generic_gin.hip -- the input-gradient variants of the generic path's one-trajectory adjoint and RHS backward.
//
// hode_generic.hip compiled a second time with HODE_GENERIC_GIN: its #ifdef HODE_GENERIC_GIN blocks add d/d{meal, tVNS, GD}
// (include/hode.h, hode_{solve,rhs}_bwd_inputs_*) to solve_bwd_generic_kernel and rhs_bwd_generic_kernel, which take other names here.
// A translation unit of its own: hipcc schedules a kernel template differently once a second variant of it shares the file, and
// the production instantiations (no input gradients) are to keep their code exactly.
#include "hode_solve_body.h"
#include <type_traits>

#define HODE_GENERIC_GIN 1
#define solve_bwd_generic_kernel solve_bwd_generic_gin_kernel
#define rhs_bwd_generic_kernel rhs_bwd_generic_gin_kernel
#define launch_rhs_bwd_generic launch_rhs_bwd_generic_gin
#include "hode_generic.hip"
