// hode_generic_bwd.hip -- the production adjoint of the generic network path: K5 (RHS backward) and the one-trajectory K4, the GIN = false
// instantiations of hode_generic_vjp.h, and the launch rule of K4 -- which team kernel a batch gets, the multi-trajectory teams of
// hode_generic_bwd_multi.hip included.  Requests for input gradients go to hode_generic_gin.hip.
#include "hode_generic_vjp.h"

namespace hode {

template <typename R> int launch_rhs_bwd_generic(hipStream_t s, const RhsArgs<R> &a, int L)
{
    if (a.gmeal || a.gtvns || a.ggd) return launch_rhs_bwd_generic_gin<R>(s, a, L);      // (hode_generic_gin.hip)
    return launch_rhs_bwd_generic_t<R, false>(s, a, L);
}

template <typename R> int launch_solve_bwd_generic(hipStream_t s, const AdjArgs<R> &a, int L, int method)
{
    if constexpr (sizeof(R) == 4) {
        // large batches: several trajectories per team (solve_bwd_generic_multi_kernel) -- needs gradient rows (one per workgroup)
        if (L >= 2 && L - 1 <= kGenAccMats && a.gnn != nullptr && a.partials != nullptr && a.n_sets <= a.partial_rows && a.n_sets <= 65535) {
            // (the fewest trajectories per team that put the batch on the chip in one round: see launch_fwd_generic_m)
            if (a.B > 1024) return launch_solve_bwd_generic_multi(s, a, L, method, 8);
            if (a.B > 512) return launch_solve_bwd_generic_multi(s, a, L, method, 4);
            if (a.B > 256) return launch_solve_bwd_generic_multi(s, a, L, method, 2);
        }
        // fp32, at most kGenAccMats hidden matrices: ALL parameter gradients accumulate in the team's registers (the wave's rows of
        // every hidden matrix, the edge pieces dealt out over the waves) and leave once per workgroup.  Teams of EIGHT waves also
        // above 64 hidden units (sixteen rows per wave: 128 accumulator registers): a 16-wave workgroup is capped at 128 VGPRs per
        // wave, which the 76 accumulators + the kernel's own ~60 registers do not fit (484 B of spills inside the stage loop).
        if (L - 1 <= kGenAccMats && a.gnn != nullptr)
            return a.H > 64 ? launch_bwd_generic_t<R, 8, 16, false>(s, a, L, method) : launch_bwd_generic_t<R, 8, 8, false>(s, a, L, method);
    }
    return a.H > 64 ? launch_bwd_generic_t<R, 16, 0, false>(s, a, L, method) : launch_bwd_generic_t<R, 8, 0, false>(s, a, L, method);
}

template int launch_rhs_bwd_generic<float>(hipStream_t, const RhsArgs<float> &, int);
template int launch_rhs_bwd_generic<double>(hipStream_t, const RhsArgs<double> &, int);
template int launch_solve_bwd_generic<float>(hipStream_t, const AdjArgs<float> &, int, int);
template int launch_solve_bwd_generic<double>(hipStream_t, const AdjArgs<double> &, int, int);

}  // namespace hode
