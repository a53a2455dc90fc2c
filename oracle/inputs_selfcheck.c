/*
 * ORACLE -- test infrastructure only.  NOT part of the product path.
 *
 * Stand-alone check of the input-gradient entry points (hode_oracle_solve_bwd_inputs_*, hode_oracle_rhs_vjp_inputs_*) and of the
 * tangent-linear one (hode_oracle_solve_jvp_*) under AddressSanitizer + UBSan: `make -C oracle selfcheck` compiles this file with the oracle sources and runs it.  One tiny case:
 * B = 2, T = 5 with a repeated time, meal on the grid, tVNS constant per trajectory, GD on the grid; every output array is
 * allocated at its exact size so that an index past a row is a sanitizer report.  Prints the sums; exit status 0 = clean run,
 * finite sums and the structural zeros in place.  The tangent pass runs on the same tape with K = 3 directions (both parts, then
 * each part alone with NULL for the other) and must be dual to the adjoint: <gy, dy> = <gx0, v_x0> + <gode, v_ode>.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define DECL(SFX, REAL)                                                                                                          \
    int hode_oracle_tape_entry_size_##SFX(void);                                                                                 \
    int hode_oracle_solve_##SFX(int, int, const REAL *, const REAL *, int, const REAL *, int, const REAL *, int, const REAL *,   \
                                int, const REAL *, const REAL *, int, int, int, double, double, int, REAL *, int *, int *,       \
                                int *, void *);                                                                                  \
    int hode_oracle_solve_bwd_inputs_##SFX(int, int, const REAL *, int, const REAL *, int, const REAL *, int, const REAL *, int, \
                                           const REAL *, const REAL *, int, int, int, int, const int *, const int *,             \
                                           const void *, const REAL *, REAL *, REAL *, REAL *, REAL *, REAL *, REAL *);          \
    int hode_oracle_solve_jvp_##SFX(int, int, const REAL *, int, const REAL *, int, const REAL *, int, const REAL *, int,        \
                                    const REAL *, const REAL *, int, int, int, int, const int *, const int *, const void *, int, \
                                    const REAL *, const REAL *, REAL *);                                                         \
    int hode_oracle_rhs_vjp_inputs_##SFX(int, const REAL *, const REAL *, const REAL *, const REAL *, const REAL *,              \
                                         const REAL *, const REAL *, int, int, const REAL *, REAL *, REAL *, REAL *, REAL *,     \
                                         REAL *, REAL *);
DECL(f32, float)
DECL(f64, double)

enum { B = 2, T = 5, H = 7, L = 2, P = 9 * H + H + (L - 1) * (H * H + H) + 6 * H + 6, MAXS = 40, KD = 3 };

static const double kOde[17] = {1.04e-2, 2.5e-2, 3e-3, 5, 60, 0.1, 50, 80, 9, 7, 2e-2, 1e-2, 1e3, 2, 5e-2, 1e-3, 1e-2};
static const double kT[T] = {0.0, 0.5, 0.5, 1.25, 2.0};            /* rows 1 and 2 repeat one time */
static const double kX0[6] = {5, 60, 80, 10, 0.5, 1};

static double lcg(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (double)(*s >> 8) / 16777216.0 - 0.5; }

static double sum_abs(const double *v, int n) { double s = 0; for (int i = 0; i < n; ++i) s += fabs(v[i]); return s; }

#define RUN(SFX, REAL)                                                                                                            \
    static int run_##SFX(int method)                                                                                              \
    {                                                                                                                             \
        unsigned seed = 12345u;                                                                                                   \
        REAL *nn = malloc(sizeof(REAL) * P), *ode = malloc(sizeof(REAL) * 17), *t = malloc(sizeof(REAL) * T);                     \
        REAL *x0 = malloc(sizeof(REAL) * B * 6), *meal = malloc(sizeof(REAL) * B * T), *tv = malloc(sizeof(REAL) * B);            \
        REAL *gd = malloc(sizeof(REAL) * B * T), *gy = malloc(sizeof(REAL) * B * T * 6), *y = malloc(sizeof(REAL) * B * T * 6);   \
        REAL *gx0 = calloc(B * 6, sizeof(REAL)), *gnn = calloc(P, sizeof(REAL)), *gode = calloc(17, sizeof(REAL));                \
        REAL *gm = calloc(B * T, sizeof(REAL)), *gt = calloc(B, sizeof(REAL)), *gg = calloc(B * T, sizeof(REAL));                 \
        int status[B], nsteps[B], nfev[B];                                                                                        \
        void *tape = calloc((size_t)B * MAXS, (size_t)hode_oracle_tape_entry_size_##SFX());                                       \
        for (int i = 0; i < P; ++i) nn[i] = (REAL)(0.2 * lcg(&seed));                                                             \
        for (int i = 0; i < 17; ++i) ode[i] = (REAL)kOde[i];                                                                      \
        for (int i = 0; i < T; ++i) t[i] = (REAL)kT[i];                                                                           \
        for (int i = 0; i < B * 6; ++i) x0[i] = (REAL)(kX0[i % 6] * (1 + 0.1 * lcg(&seed)));                                      \
        for (int i = 0; i < B * T; ++i) { meal[i] = (REAL)(1.5 + lcg(&seed)); gd[i] = (REAL)(500 + 400 * lcg(&seed)); }           \
        for (int i = 0; i < B; ++i) tv[i] = (REAL)(0.5 + lcg(&seed));                                                             \
        for (int i = 0; i < B * T * 6; ++i) gy[i] = (REAL)lcg(&seed);                                                             \
        int rc = hode_oracle_solve_##SFX(B, T, x0, t, 0, meal, 2, tv, 1, gd, 2, ode, nn, H, L, method, 1e-6, 1e-8, MAXS, y,       \
                                         status, nsteps, nfev, tape);                                                             \
        if (rc == 0)                                                                                                              \
            rc = hode_oracle_solve_bwd_inputs_##SFX(B, T, t, 0, meal, 2, tv, 1, gd, 2, ode, nn, H, L, method, MAXS, nsteps,       \
                                                    status, tape, gy, gx0, gnn, gode, gm, gt, gg);                                \
        double sm[B * T], st[B], sg[B * T];                                                                                       \
        for (int i = 0; i < B * T; ++i) { sm[i] = (double)gm[i]; sg[i] = (double)gg[i]; }                                         \
        for (int i = 0; i < B; ++i) st[i] = (double)gt[i];                                                                        \
        double a = sum_abs(sm, B * T), b = sum_abs(st, B), c = sum_abs(sg, B * T);                                                \
        printf(#SFX " method %d: status %d %d  nsteps %d %d  |g_meal| %.9g  |g_tVNS| %.9g  |g_GD| %.9g\n", method, status[0],    \
               status[1], nsteps[0], nsteps[1], a, b, c);                                                                         \
        int bad = rc != 0 || status[0] != 0 || status[1] != 0 || !(a > 0) || !(b > 0) || !(c > 0) || !isfinite(a + b + c);        \
        /* the tangent pass over the same tape: both parts, then each alone; dual to the adjoint above */                         \
        REAL *vo = malloc(sizeof(REAL) * KD * 17), *vx = malloc(sizeof(REAL) * B * KD * 6);                                       \
        REAL *dy = malloc(sizeof(REAL) * B * KD * T * 6), *dyo = malloc(sizeof(REAL) * B * KD * T * 6);                           \
        REAL *dyx = malloc(sizeof(REAL) * B * KD * T * 6);                                                                        \
        for (int i = 0; i < KD * 17; ++i) vo[i] = (REAL)(kOde[i % 17] * lcg(&seed));                                              \
        for (int i = 0; i < B * KD * 6; ++i) vx[i] = (REAL)(kX0[i % 6] * lcg(&seed));                                             \
        rc = hode_oracle_solve_jvp_##SFX(B, T, t, 0, meal, 2, tv, 1, gd, 2, ode, nn, H, L, method, MAXS, nsteps, status, tape,    \
                                         KD, vo, vx, dy);                                                                         \
        rc |= hode_oracle_solve_jvp_##SFX(B, T, t, 0, meal, 2, tv, 1, gd, 2, ode, nn, H, L, method, MAXS, nsteps, status, tape,   \
                                          KD, vo, NULL, dyo);                                                                     \
        rc |= hode_oracle_solve_jvp_##SFX(B, T, t, 0, meal, 2, tv, 1, gd, 2, ode, nn, H, L, method, MAXS, nsteps, status, tape,   \
                                          KD, NULL, vx, dyx);                                                                     \
        double worst = 0, split = 0;                                                                                              \
        for (int k = 0; k < KD; ++k) {                                                                                            \
            double lhs = 0, rhs = 0, sc = 0;                                                                                      \
            for (int b = 0; b < B; ++b) {                                                                                         \
                for (int i = 0; i < T * 6; ++i) {                                                                                 \
                    double q = (double)gy[b * T * 6 + i] * (double)dy[(b * KD + k) * T * 6 + i];                                  \
                    lhs += q; sc += fabs(q);                                                                                      \
                    double lin = (double)dyo[(b * KD + k) * T * 6 + i] + (double)dyx[(b * KD + k) * T * 6 + i];                   \
                    split = fmax(split, fabs(lin - (double)dy[(b * KD + k) * T * 6 + i]) /                                        \
                                            (fabs((double)dy[(b * KD + k) * T * 6 + i]) + 1.0));                                  \
                }                                                                                                                 \
                for (int i = 0; i < 6; ++i) {                                                                                     \
                    double q = (double)gx0[b * 6 + i] * (double)vx[(b * KD + k) * 6 + i];                                         \
                    rhs += q; sc += fabs(q);                                                                                      \
                    bad |= dy[(b * KD + k) * T * 6 + i] != vx[(b * KD + k) * 6 + i] || dyo[(b * KD + k) * T * 6 + i] != 0;        \
                    bad |= dy[((b * KD + k) * T + 2) * 6 + i] != dy[((b * KD + k) * T + 1) * 6 + i];   /* the repeated time */   \
                }                                                                                                                 \
            }                                                                                                                     \
            for (int i = 0; i < 17; ++i) { double q = (double)gode[i] * (double)vo[k * 17 + i]; rhs += q; sc += fabs(q); }        \
            worst = fmax(worst, fabs(lhs - rhs) / sc);                                                                            \
        }                                                                                                                         \
        const double dual_tol = sizeof(REAL) == 8 ? 1e-12 : 1e-4, split_tol = sizeof(REAL) == 8 ? 1e-12 : 1e-4;                   \
        printf(#SFX " method %d: jvp duality %.3g  v_ode-only + v_x0-only against both %.3g\n", method, worst, split);            \
        bad |= rc != 0 || !(worst <= dual_tol) || !(split <= split_tol);                                                          \
        free(vo); free(vx); free(dy); free(dyo); free(dyx);                                                                       \
        /* RHS entry point: one sample with GD > 0, one with GD = 0 (gradient exactly 0), meal alone wanted for the check below */\
        REAL rx[B * 6], rt[B] = {0, 1}, rm[B] = {1, 2}, rv[B] = {0.25f, 0.75f}, rg[B] = {600, 0}, rw[B * 6], rgx[B * 6];          \
        REAL rgm[B] = {0, 0}, rgt[B] = {0, 0}, rgg[B] = {0, 0};                                                                   \
        for (int i = 0; i < B * 6; ++i) { rx[i] = x0[i]; rw[i] = (REAL)(1 + lcg(&seed)); }                                        \
        rc = hode_oracle_rhs_vjp_inputs_##SFX(B, rx, rt, rm, rv, rg, ode, nn, H, L, rw, rgx, NULL, NULL, rgm, rgt, rgg);          \
        printf(#SFX " rhs: g_meal %.9g %.9g  g_tVNS %.9g %.9g  g_GD %.9g %.9g\n", (double)rgm[0], (double)rgm[1],               \
               (double)rgt[0], (double)rgt[1], (double)rgg[0], (double)rgg[1]);                                                   \
        bad |= rc != 0 || rgm[0] != rw[0] || rgm[1] != rw[6] || rgg[0] == 0 || rgg[1] != 0 || rgt[0] == 0;                        \
        rc = hode_oracle_rhs_vjp_inputs_##SFX(B, rx, rt, rm, NULL, NULL, ode, nn, H, L, rw, rgx, gnn, gode, rgm, NULL, NULL);     \
        bad |= rc != 0 || rgm[0] != rw[0];                                                                                        \
        free(nn); free(ode); free(t); free(x0); free(meal); free(tv); free(gd); free(gy); free(y); free(gx0); free(gnn);          \
        free(gode); free(gm); free(gt); free(gg); free(tape);                                                                     \
        return bad;                                                                                                               \
    }
RUN(f32, float)
RUN(f64, double)

int main(void)
{
    int bad = 0;
    for (int method = 0; method < 2; ++method) bad |= run_f32(method) | run_f64(method);
    printf(bad ? "inputs_selfcheck: FAILED\n" : "inputs_selfcheck: ok\n");
    printf(bad ? "jvp_selfcheck: FAILED\n" : "jvp_selfcheck: ok\n");
    return bad;
}
