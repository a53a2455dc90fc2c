// hode_tableau.h -- the Runge-Kutta tableaux as device data and the two LDS coefficient-row stores.
// Used by: hode_solve_body.h (the forward solves), hode_solve_jvp.hip, hode_solve_bwd.hip, hode_solve_bwd_ws.hip, hode_generic_vjp.h,
// hode_generic_bwd_multi.hip, lab/hode_solve_bwd_split.hip.
#pragma once
#include "hode_xlane.h"
#include "../../include/hode.h"

namespace hode {

// ------------------------------------------------------------------------------------------
// Runge-Kutta tableaux as data.  The stage derivatives of a step are PACKED into one VGPR:
// lanes 8s..8s+7 hold stage s (component = lane & 7), so a stage combination
//   Y_s = Y + h * sum_j a_sj K_j   is   Y + h * group_sum8(coef_s * KK)
// with a per-lane coefficient row coef_s[lane] = a[s][lane >> 3] fetched from an LDS table.
// One copy of the RHS code serves every stage (the stage loop is NOT unrolled).
struct TableauData {
    double A[8][8];   // A[s][j]; for DP5(4) row 6 = the 5th-order weights (FSAL stage)
    double bw[8];     // solution weights
    double c[8];      // nodes
    double E[8];      // error-estimate weights (DP5(4) only)
    int S;            // stages that carry the solution (backward sweeps these)
};
__constant__ TableauData kTableau[2] = {
    // HODE_METHOD_DP54: Dormand-Prince 5(4) (scipy/integrate/_ivp/rk.py:377-401)
    {{{0},
      {1.0 / 5},
      {3.0 / 40, 9.0 / 40},
      {44.0 / 45, -56.0 / 15, 32.0 / 9},
      {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
      {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
      {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84},
      {0}},
     {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0, 0},
     {0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1, 1, 0},
     {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40, 0},
     6},
    // HODE_METHOD_RK4: the classic 4-stage scheme
    {{{0}, {0.5}, {0, 0.5}, {0, 0, 1.0}, {0}, {0}, {0}, {0}},
     {1.0 / 6, 2.0 / 6, 2.0 / 6, 1.0 / 6, 0, 0, 0, 0},
     {0, 0.5, 0.5, 1.0, 0, 0, 0, 0},
     {0},
     4}};

// LDS coefficient rows (per workgroup): rowsA[s][lane] = A[s][lane>>3]; row 7 = E (DP) / bw (RK4)
template <typename R> __device__ __forceinline__ void tableau_rows_store(R *rows, int method, int tid, int nthreads)
{
    for (int i = tid; i < 8 * kWave; i += nthreads) {
        const int s = i >> 6, l = i & 63;
        double v = kTableau[method].A[s][l >> 3];
        if (s == 7) v = (method == HODE_METHOD_DP54) ? kTableau[method].E[l >> 3] : kTableau[method].bw[l >> 3];
        rows[i] = (R)v;
    }
}
// transposed rows for the adjoint: rowsT[s][lane] = A[lane>>3][s] (only stages < S); row 7 = 1 for stages < S;
// row 6 carries the solution weights bw[0..7] (lanes 0..7) and the nodes c[0..7] (lanes 8..15) as reals
template <typename R> __device__ __forceinline__ void tableau_rowsT_store(R *rows, int method, int tid, int nthreads)
{
    const int S = kTableau[method].S;
    for (int i = tid; i < 8 * kWave; i += nthreads) {
        const int s = i >> 6, l = i & 63, j = l >> 3;
        double v = (j < S && s < S) ? kTableau[method].A[j][s] : 0.0;
        if (s == 7) v = (j < S) ? 1.0 : 0.0;
        if (s == 6) v = (l < 8) ? kTableau[method].bw[l] : (l < 16) ? kTableau[method].c[l - 8] : 0.0;   // scalars as reals
        rows[i] = (R)v;
    }
}

}  // namespace hode
