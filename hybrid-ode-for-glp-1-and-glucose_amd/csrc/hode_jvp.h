// hode_jvp.h -- the mechanistic half of the tangent-linear pass: what hode_solve_jvp.hip (tuned shapes, one trajectory per wave)
// and hode_generic_jvp.hip (generic networks, one trajectory per team) share.  The network half differs between the two.
#pragma once
#include "hode_rhs_eval.h"

namespace hode {

// The ODE constants whose derivative the lane's component c8 has, in the order of jvp_coeffs below (-1: none).
//   G: k_GE0, I_b, Glu_b, IGD_50, g    I: a_GI, k_I, rho, G_b, I_b    Glu: E_max, EC_50, Glu_b    GLP1: V_max, K_m, k_L
//   FFA: p_7, p_8, p_9                 GE (no dynamics) and the padding slots: none
__constant__ signed char kJvpPar[8][5] = {{11, 4, 7, 12, 13}, {0, 1, 2, 3, 4}, {5, 6, 7, -1, -1}, {8, 9, 10, -1, -1},
                                          {-1, -1, -1, -1, -1}, {14, 15, 16, -1, -1}, {-1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1}};

// Row c8 of the mechanistic Jacobian at the stage state (models/ode_core.py:124-153; the transpose of mech_vjp):
//   js[0..4]  d f_c8 / d (G, I, Glu, GLP1, FFA)           (GE enters no mechanistic term)
//   jp[0..4]  d f_c8 / d (the constants kJvpPar[c8])
// GD: the Hill term's constants IGD_50 and g act through k_GE = k_GE0 (1 - gde(GD)); zero derivative at GD <= 0, as in the adjoint.
template <typename R, bool GD>
__device__ __forceinline__ void jvp_coeffs(const OdeP<R> &o, R G, R I, R Glu, R GLP1, R FFA, R gde, R gdv, int c8, R (&js)[5],
                                           R (&jp)[5])
{
    const R u = G - o.G_b, vI = I - o.I_b, w = Glu - o.Glu_b;
    const R Pi = R(1) + o.rho * GLP1;
    const R r1 = rdiv(R(1), o.EC_50 + GLP1), r2 = rdiv(R(1), o.K_m + G);
    const R k_GE = o.k_GE0 * (R(1) - gde);
    R g12 = R(0), g13 = R(0);
    if constexpr (GD) {
        if (gdv > R(0)) {
            const R uu = rpow(gdv, o.g), vv = rpow(o.IGD_50, o.g), s2 = (vv + uu) * (vv + uu);
            g12 = o.k_GE0 * G * (-uu * o.g * rpow(o.IGD_50, o.g - R(1)) / s2);
            g13 = o.k_GE0 * G * (uu * vv * (rlog(gdv) - rlog(o.IGD_50)) / s2);
        }
    }
    const R eg = o.E_max * GLP1 * r1;
    const R z = R(0);
    // (a select per coefficient on every lane: the lane's component is a lane property, the values are shared)
    const bool cG = c8 == 0, cI = c8 == 1, cU = c8 == 2, cP = c8 == 3, cF = c8 == 5;
    js[0] = cG ? -k_GE : cI ? Pi * o.a_GI : cP ? o.V_max * o.K_m * r2 * r2 : cF ? o.p_9 * FFA : z;
    js[1] = cG ? R(-0.01) : cI ? -o.k_I : cF ? -o.p_8 * FFA : z;
    js[2] = cG ? R(0.005) : cU ? -eg : z;
    js[3] = cI ? o.rho * o.a_GI * u : cU ? -o.E_max * o.EC_50 * r1 * r1 * w : cP ? -o.k_L : z;
    js[4] = cF ? (-o.p_7 - o.p_8 * I + o.p_9 * G) : z;
    jp[0] = cG ? -G * (R(1) - gde) : cI ? Pi * u : cU ? -GLP1 * r1 * w : cP ? G * r2 : cF ? -FFA : z;
    jp[1] = cG ? R(0.01) : cI ? -vI : cU ? eg * r1 * w : cP ? -o.V_max * G * r2 * r2 : cF ? -I * FFA : z;
    jp[2] = cG ? R(-0.005) : cI ? GLP1 * o.a_GI * u : cU ? eg : cP ? -GLP1 : cF ? G * FFA : z;
    jp[3] = cG ? g12 : cI ? -Pi * o.a_GI : z;
    jp[4] = cG ? g13 : cI ? o.k_I : z;
}

}  // namespace hode
