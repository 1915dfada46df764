// state_estimator.hip -- the state estimator between the env step and the control step (gfx950): covo_estimate /
// covo_set_step_estimator, include/covo_hip.h; DESIGN.md 4.33.
//
// An extended Kalman filter on the model the rollouts use (quad_model.hpp, fp64), measurement = the full 13-coordinate state (H = I).
// Per instance it keeps x [13] (pos, vel, quat, omega), P [13][13] (symmetric bit for bit), the force f_prev and the time word t_prev
// of the row it last saw, and a valid bit.  A call with the measured row z [32] and the applied action u [4]:
//   init     no valid state, or time(z) != t_prev + 1 (an auto-reset, an episode end): x = (double)z[0:13], P = R; the row stays
//   predict  x- = f(x, clip(u), f_prev), A = df/dx at x from 13 forward tangents (qm::D1), P- = A P A^T + Q
//   update   S = P- + R = L D L^T (unpivoted; the pivots D are the squares of the Cholesky factor's diagonal), nu = z - x-,
//            K = (S^-1 P-)^T by the two triangular solves, x = x- + K nu,
//            P = (I - K) P- (I - K)^T + K R K^T (Joseph), every row computed, the lower triangle mirrored
//   write    row[0:13] = fp32(x) -- nothing else of the row --, f_prev = z.f_disturb, t_prev = time(z)
// Decided on the device, reported in the side row, none an error:
//   bit 0  initialised: no valid state                   bit 1  re-initialised: the time word
//   bit 2  one of the 13 measured coordinates is not finite: the row is untouched, the filter is invalidated
//   bit 3  a pivot of S is not positive and finite, or x / P has an entry that is not finite: re-initialised from z, the row untouched
//   side row  float[8] = {bits(flags), nu^T S^-1 nu, |nu_pos|, |x - z|_pos, P00 + P11 + P22, P33 + P44 + P55, smallest pivot, bits(time)}
//             (an initialisation: 0 for entries 1 .. 3 and 6; bit 2: 0 for entries 1 .. 6)
//
// One launch, one workgroup of ONE wave per instance; the aim is latency.  Every load -- the row, u, x, f_prev, the lane's row of P,
// the two meta words -- is issued before the first use; the model and the variances travel in the argument block.  Lane j < 13
// carries tangent j through the model step (the primal parts repeat each other: x- is known to every lane) and then row / column j of
// every matrix in registers; an entry another lane holds arrives by v_readlane (a wave-uniform operand of the fma), so every
// register index is a constant and nothing spills.  Two 13 x 13 transposes (P A^T, and the mirror of the Joseph form) go through
// 1.4 KB of LDS (two passes).  Lane 13 carries nu through the solves as one more right-hand side: nu^T S^-1 nu.  Lanes 14 .. 63 repeat lane 12
// and store nothing.  Batched instances take their argument block from device memory, pointers through rebase_global, as
// plan_hold_kernel does; the log's row index is a kernel argument, so the blocks of a steady-state episode never change.
#include "after_step.hpp"
#include "wave_reduce.hpp"

constexpr int SE_BLOCK = COVO_WAVE;
constexpr int SE_NX = 13;
constexpr int SE_LD = SE_NX;  // leading dimension of the transposes in LDS (odd: rows on different banks)

__device__ __forceinline__ bool se_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)
__device__ __forceinline__ int se_group(int c) { return c < 3 ? 0 : (c < 6 ? 1 : (c < 10 ? 2 : 3)); }

// v[m] of lane l -> out[m] of lane m ... that is out[m] (lane l) = v[l] (lane m), through LDS; lanes >= 13 take lane 12's part
__device__ __forceinline__ void se_transpose(const double (&v)[SE_NX], double (&out)[SE_NX], double *lds, int lane, int r)
{
    __syncthreads();  // (one wave: the reads of the previous transpose are done)
    if (lane < SE_NX) {
#pragma unroll
        for (int m = 0; m < SE_NX; ++m) lds[m * SE_LD + lane] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < SE_NX; ++m) out[m] = lds[r * SE_LD + m];
}

template <bool BATCHED>
__global__ __launch_bounds__(SE_BLOCK) void state_estimator_kernel(const EstDesc D_, const EstDesc *__restrict__ batch, const int fresh,
                                                                   const int log_index)
{
    __shared__ double se_lds[SE_NX * SE_LD];
    EstDesc Db;
    if (BATCHED) {
        Db = batch[blockIdx.x];
        Db.state = rebase_global(D_.state, Db.state);
        Db.u = rebase_global(D_.u, Db.u);
        Db.xhat = rebase_global(D_.xhat, Db.xhat);
        Db.P = rebase_global(D_.P, Db.P);
        Db.meta = rebase_global(D_.meta, Db.meta);
        Db.row_out = rebase_global(D_.row_out, Db.row_out);
        Db.log = rebase_global(D_.log, Db.log);
    }
    const EstDesc &D = BATCHED ? Db : D_;
    const int lane = threadIdx.x, r = lane < SE_NX ? lane : SE_NX - 1;

    // ---- every load
    float *__restrict__ st = D.state;
    float zf[SE_NX], ff[3], uf[4];
#pragma unroll
    for (int c = 0; c < SE_NX; ++c) zf[c] = st[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) ff[c] = st[ST_FDIST + c];
    const int t_z = reinterpret_cast<const int *>(st)[ST_TIME];
#pragma unroll
    for (int c = 0; c < 4; ++c) uf[c] = D.u[c];
    double x[SE_NX], fp[3], p[SE_NX];
#pragma unroll
    for (int c = 0; c < SE_NX; ++c) x[c] = D.xhat[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) fp[c] = D.xhat[SE_NX + c];
#pragma unroll
    for (int c = 0; c < SE_NX; ++c) p[c] = D.P[r * SE_NX + c];  // row r of P = its column r
    const int valid = fresh ? 0 : D.meta[0];
    const int t_prev = D.meta[1];

    double z[SE_NX];
    bool zfin = true;
#pragma unroll
    for (int c = 0; c < SE_NX; ++c) {
        z[c] = (double)zf[c];
        zfin = zfin && se_finite(z[c]);
    }
    const bool jump = valid != 0 && t_z != t_prev + 1;
    const bool run = zfin && valid != 0 && !jump;  // (wave-uniform)
    // the lane's own entries of the uniform vectors
    const double R_r = r < 3 ? D.R[0] : (r < 6 ? D.R[1] : (r < 10 ? D.R[2] : D.R[3]));
    const double Q_r = r < 3 ? D.Q[0] : (r < 6 ? D.Q[1] : (r < 10 ? D.Q[2] : D.Q[3]));
    double z_r = z[0];
#pragma unroll
    for (int c = 1; c < SE_NX; ++c) z_r = r == c ? z[c] : z_r;

    bool ok = run;
    double x_new = z_r, pn[SE_NX], nis = 0.0, innov = 0.0, dmin = 0.0;
#pragma unroll
    for (int m = 0; m < SE_NX; ++m) pn[m] = r == m ? R_r : 0.0;
    if (run) {
        // ---- predict: the model step on tangent r
        qm::State<qm::D1> s;
        s.px = qm::D1{x[0], r == 0 ? 1.0 : 0.0};
        s.py = qm::D1{x[1], r == 1 ? 1.0 : 0.0};
        s.pz = qm::D1{x[2], r == 2 ? 1.0 : 0.0};
        s.vx = qm::D1{x[3], r == 3 ? 1.0 : 0.0};
        s.vy = qm::D1{x[4], r == 4 ? 1.0 : 0.0};
        s.vz = qm::D1{x[5], r == 5 ? 1.0 : 0.0};
        s.qx = qm::D1{x[6], r == 6 ? 1.0 : 0.0};
        s.qy = qm::D1{x[7], r == 7 ? 1.0 : 0.0};
        s.qz = qm::D1{x[8], r == 8 ? 1.0 : 0.0};
        s.qw = qm::D1{x[9], r == 9 ? 1.0 : 0.0};
        s.ox = qm::D1{x[10], r == 10 ? 1.0 : 0.0};
        s.oy = qm::D1{x[11], r == 11 ? 1.0 : 0.0};
        s.oz = qm::D1{x[12], r == 12 ? 1.0 : 0.0};
        const qm::D1 a0{qm::clip11_((double)uf[0]), 0.0}, a1{qm::clip11_((double)uf[1]), 0.0}, a2{qm::clip11_((double)uf[2]), 0.0},
            a3{qm::clip11_((double)uf[3]), 0.0};
        qm::dyn_step<qm::D1, double, true, double>(s, a0, a1, a2, a3, D.c, fp[0], fp[1], fp[2]);
        const double xm[SE_NX] = {s.px.v, s.py.v, s.pz.v, s.vx.v, s.vy.v, s.vz.v, s.qx.v, s.qy.v, s.qz.v, s.qw.v, s.ox.v, s.oy.v, s.oz.v};
        const double a[SE_NX] = {s.px.a, s.py.a, s.pz.a, s.vx.a, s.vy.a, s.vz.a, s.qx.a, s.qy.a, s.qz.a, s.qw.a, s.ox.a, s.oy.a, s.oz.a};
        // a[i] (lane k) = A[i][k].  W = P A^T: w[l] (lane j) = W[j][l] = sum_k P[j][k] A[l][k]
        double w[SE_NX];
#pragma unroll
        for (int l = 0; l < SE_NX; ++l) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < SE_NX; ++k) acc = fma(p[k], wr::bcast_lane(a[l], k), acc);
            w[l] = acc;
        }
        double wt[SE_NX];  // wt[k] (lane l) = W[k][l]
        se_transpose(w, wt, se_lds, lane, r);
        // P- = A W + Q: pm[i] (lane l) = P-[i][l]
        double pm[SE_NX];
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) {
            double acc = r == i ? Q_r : 0.0;
#pragma unroll
            for (int k = 0; k < SE_NX; ++k) acc = fma(wr::bcast_lane(a[i], k), wt[k], acc);
            pm[i] = acc;
        }
        // ---- S = P- + R = L D L^T by symmetric elimination: sc[i] (lane l) = S[i][l]; after step k lane l > k holds L[l][k] in lk[k]
        double sc[SE_NX], lk[SE_NX], dk[SE_NX];
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) sc[i] = pm[i] + (r == i ? R_r : 0.0);
        dmin = __builtin_inf();
#pragma unroll
        for (int k = 0; k < SE_NX; ++k) {
            const double d = wr::bcast_lane(sc[k], k);
            ok = ok && d > 0.0 && se_finite(d);
            dmin = fmin(dmin, d);
            dk[k] = qm::rcp64_(d);
            const double f = sc[k] * dk[k];  // S[k][l] / d = L[l][k] (by symmetry the lane's own entry)
            lk[k] = f;
#pragma unroll
            for (int i = k + 1; i < SE_NX; ++i) sc[i] = fma(-wr::bcast_lane(sc[i], k), f, sc[i]);
        }
        // ---- the solves: lane l < 13 with column l of P-, lane 13 with nu; y = S^-1 b
        double nu[SE_NX], y[SE_NX];
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) nu[i] = z[i] - xm[i];
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) y[i] = lane == SE_NX ? nu[i] : pm[i];
#pragma unroll
        for (int i = 1; i < SE_NX; ++i) {
#pragma unroll
            for (int k = 0; k < i; ++k) y[i] = fma(-wr::bcast_lane(lk[k], i), y[k], y[i]);
        }
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) y[i] *= dk[i];
#pragma unroll
        for (int i = SE_NX - 2; i >= 0; --i) {
#pragma unroll
            for (int k = i + 1; k < SE_NX; ++k) y[i] = fma(-wr::bcast_lane(lk[i], k), y[k], y[i]);
        }
        // lane l < 13: y[i] = (S^-1 P-)[i][l] = K[l][i]; lane 13: S^-1 nu
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) dot = fma(y[i], nu[i], dot);
        nis = wr::bcast_lane(dot, SE_NX);
        innov = sqrt(fma(nu[2], nu[2], fma(nu[1], nu[1], nu[0] * nu[0])));
        double xm_r = xm[0];
#pragma unroll
        for (int c = 1; c < SE_NX; ++c) xm_r = r == c ? xm[c] : xm_r;
        x_new = xm_r + dot;
        // ---- Joseph: G = I - K (row l in lane l), T = G P-, P = T G^T + K R K^T
        double g[SE_NX], t[SE_NX], kr[SE_NX];
#pragma unroll
        for (int i = 0; i < SE_NX; ++i) {
            g[i] = (r == i ? 1.0 : 0.0) - y[i];
            kr[i] = y[i] * D.R[se_group(i)];
        }
#pragma unroll
        for (int j = 0; j < SE_NX; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < SE_NX; ++i) acc = fma(g[i], wr::bcast_lane(pm[i], j), acc);
            t[j] = acc;
        }
        double full[SE_NX], mirror[SE_NX];
#pragma unroll
        for (int m = 0; m < SE_NX; ++m) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < SE_NX; ++j) acc = fma(t[j], wr::bcast_lane(g[j], m), acc);
#pragma unroll
            for (int j = 0; j < SE_NX; ++j) acc = fma(kr[j], wr::bcast_lane(y[j], m), acc);
            full[m] = acc;
        }
        se_transpose(full, mirror, se_lds, lane, r);
        bool fin = se_finite(x_new);
#pragma unroll
        for (int m = 0; m < SE_NX; ++m) {
            pn[m] = m <= r ? full[m] : mirror[m];
            fin = fin && se_finite(pn[m]);
        }
        ok = ok && __all((fin || lane == SE_NX) ? 1 : 0) != 0;  // (lane 13 carried nu, not a column of P-)
        if (!ok) {  // (uniform) as an initialisation
            x_new = z_r;
#pragma unroll
            for (int m = 0; m < SE_NX; ++m) pn[m] = r == m ? R_r : 0.0;
            nis = innov = dmin = 0.0;
        }
    }
    const int flags = !zfin ? 4 : (valid == 0 ? 1 : (jump ? 2 : (ok ? 0 : 8)));
    // the row's statistics: the estimate's first three entries and the diagonal of P live in lanes 0 .. 5
    const double e0 = wr::bcast_lane(x_new, 0) - z[0], e1 = wr::bcast_lane(x_new, 1) - z[1], e2 = wr::bcast_lane(x_new, 2) - z[2];
    const double moved = sqrt(fma(e2, e2, fma(e1, e1, e0 * e0)));
    const double tr_pos = wr::bcast_lane(pn[0], 0) + wr::bcast_lane(pn[1], 1) + wr::bcast_lane(pn[2], 2);
    const double tr_vel = wr::bcast_lane(pn[3], 3) + wr::bcast_lane(pn[4], 4) + wr::bcast_lane(pn[5], 5);

    // ---- stores
    const float x32 = (float)x_new;
    const bool wrote = zfin && ok;  // the row receives the estimate
    if (zfin) {
        if (lane < SE_NX) {
            D.xhat[lane] = x_new;
#pragma unroll
            for (int m = 0; m < SE_NX; ++m) D.P[lane * SE_NX + m] = pn[m];
            if (ok) st[lane] = x32;
        } else if (lane < SE_NX + 3) {
            D.xhat[lane] = lane == SE_NX ? (double)ff[0] : (lane == SE_NX + 1 ? (double)ff[1] : (double)ff[2]);
        } else if (lane == SE_NX + 3) {
            D.meta[0] = 1;
            D.meta[1] = t_z;
        }
    } else if (lane == SE_NX + 3) {
        D.meta[0] = 0;
    }
    float w8 = 0.0f;
    if (lane < COVO_EST_FLOATS) {
        const bool stats = zfin;
        w8 = lane == 0   ? __int_as_float(flags)
             : lane == 1 ? (float)nis
             : lane == 2 ? (float)innov
             : lane == 3 ? (stats ? (float)moved : 0.0f)
             : lane == 4 ? (stats ? (float)tr_pos : 0.0f)
             : lane == 5 ? (stats ? (float)tr_vel : 0.0f)
             : lane == 6 ? (float)dmin
                         : __int_as_float(t_z);
        if (D_.row_out != nullptr) D.row_out[lane] = w8;
    }
    if (D_.log != nullptr && log_index >= 0) {
        float *lg = D.log + (size_t)log_index * COVO_EST_LOG_FLOATS;
        if (lane < SE_NX) {
            float zl = zf[0];
#pragma unroll
            for (int c = 1; c < SE_NX; ++c) zl = lane == c ? zf[c] : zl;
            lg[lane] = zl;
            lg[SE_NX + lane] = wrote ? x32 : zl;
        }
        if (lane < COVO_EST_FLOATS) lg[2 * SE_NX + lane] = w8;
    }
}

// ---- host
int estimator_fill_model(EstDesc &d, const covo_env_params &p, const double *obs_std, const double *proc_std, double force_std, const char *what)
{
    const double inf = __builtin_inf();
    for (int g = 0; g < 4; ++g) {
        REQUIRE(obs_std[g] > 0.0 && obs_std[g] < inf, "%s: obs_std[%d]=%g is not a positive finite number", what, g, obs_std[g]);
        const bool derive = g == 1 && proc_std[g] < 0.0;
        REQUIRE(derive || (proc_std[g] >= 0.0 && proc_std[g] < inf), "%s: proc_std[%d]=%g is not a finite number >= 0%s", what, g,
                proc_std[g], g == 1 ? " (a negative velocity entry derives it from force_std)" : "");
        REQUIRE(!derive || (force_std >= 0.0 && force_std < inf), "%s: force_std=%g is not a finite number >= 0", what, force_std);
        const double q = derive ? (double)p.dt * force_std / (double)p.m : proc_std[g];
        d.R[g] = obs_std[g] * obs_std[g];
        d.Q[g] = q * q;
    }
    d.c = make_consts<double>(p);
    return 0;
}

int launch_state_estimator(covo_ctx *h, const EstDesc *d, int n_inst, bool batched, bool primitive, int fresh, int log_index, hipStream_t s)
{
    if (n_inst < 1 || n_inst > COVO_MAX_ENVS) {
        covo_set_error("state estimator: n_inst=%d outside (0, %d]", n_inst, COVO_MAX_ENVS);
        return COVO_E_BADARG;
    }
    if (!batched) {
        hipLaunchKernelGGL(state_estimator_kernel<false>, dim3(1), dim3(SE_BLOCK), 0, s, d[0], (const EstDesc *)nullptr, fresh, log_index);
    } else {
        ArgBlockCache &c = primitive ? after_state(h)->est_primitive : after_state(h)->est;
        if (int rc = c.sync_upload(d, (size_t)n_inst * sizeof(EstDesc), sizeof(EstDesc), s)) return rc;
        hipLaunchKernelGGL(state_estimator_kernel<true>, dim3(n_inst), dim3(SE_BLOCK), 0, s, d[0], (const EstDesc *)c.dev, fresh, log_index);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int covo_estimator_step(covo_ctx *h, float *states, const float *a_mean, const covo_env_params *params, int n_inst, bool batched,
                        int log_index, hipStream_t s)
{
    if (!covo_estimator_on(h)) return 0;
    static thread_local EstDesc d[COVO_MAX_ENVS];
    std::memset(d, 0, (size_t)n_inst * sizeof(EstDesc));
    for (int e = 0; e < n_inst; ++e) {
        if (int rc = estimator_fill_model(d[e], params[e], h->est_obs_std, h->est_proc_std, h->est_force_std, "covo_set_step_estimator")) return rc;
        d[e].state = states + (size_t)e * COVO_STATE_FLOATS;
        d[e].u = a_mean + (size_t)e * COVO_NA;
        d[e].xhat = h->est_xhat + (size_t)e * COVO_EST_STATE_DOUBLES;
        d[e].P = h->est_P + (size_t)e * SE_NX * SE_NX;
        d[e].meta = h->est_meta + (size_t)e * COVO_EST_META_INTS;
        d[e].row_out = h->est_rows + (size_t)e * COVO_EST_FLOATS;
        d[e].log = h->est_log ? h->est_log + (size_t)e * h->est_log_stride * COVO_EST_LOG_FLOATS : nullptr;
    }
    const int fresh = h->est_fresh;
    h->est_fresh = 0;
    return launch_state_estimator(h, d, n_inst, batched, false, fresh, log_index, s);
}
