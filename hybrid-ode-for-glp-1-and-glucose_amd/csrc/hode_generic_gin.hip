// hode_generic_gin.hip -- the input-gradient variants of the generic path's one-trajectory adjoint and RHS backward: the GIN = true
// instantiations of solve_bwd_generic_kernel and rhs_bwd_generic_kernel (hode_generic_vjp.h), which add d/d{meal, tVNS, GD}
// (include/hode.h, hode_{solve,rhs}_bwd_inputs_*).
// A translation unit of its own: hipcc schedules a kernel template differently once a second variant of it shares the file, and
// the production instantiations (no input gradients, hode_generic_bwd.hip) are to keep their code exactly.
#include "hode_generic_vjp.h"

namespace hode {

template <typename R> int launch_rhs_bwd_generic_gin(hipStream_t s, const RhsArgs<R> &a, int L)
{
    return launch_rhs_bwd_generic_t<R, true>(s, a, L);
}

// input gradients: the one-trajectory teams for every batch (register accumulators where the production path has them, atomics
// elsewhere -- the same families as launch_solve_bwd_generic, without the multi-trajectory teams)
template <typename R> int launch_solve_bwd_generic_gin(hipStream_t s, const AdjInArgs<R> &a, int L, int method)
{
    if constexpr (sizeof(R) == 4) {
        if (L - 1 <= kGenAccMats && a.gnn != nullptr)
            return a.H > 64 ? launch_bwd_generic_t<R, 8, 16, true>(s, a, L, method) : launch_bwd_generic_t<R, 8, 8, true>(s, a, L, method);
    }
    return a.H > 64 ? launch_bwd_generic_t<R, 16, 0, true>(s, a, L, method) : launch_bwd_generic_t<R, 8, 0, true>(s, a, L, method);
}

template int launch_rhs_bwd_generic_gin<float>(hipStream_t, const RhsArgs<float> &, int);
template int launch_rhs_bwd_generic_gin<double>(hipStream_t, const RhsArgs<double> &, int);
template int launch_solve_bwd_generic_gin<float>(hipStream_t, const AdjInArgs<float> &, int, int);
template int launch_solve_bwd_generic_gin<double>(hipStream_t, const AdjInArgs<double> &, int, int);

}  // namespace hode
