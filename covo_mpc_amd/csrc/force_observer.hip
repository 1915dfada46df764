// force_observer.hip -- the force observer between the env step and the control step (gfx950): covo_observe_force /
// covo_set_step_force_observer, include/covo_hip.h; DESIGN.md 4.34.
//
// An extended Kalman filter on the model the rollouts use (quad_model.hpp, fp64) whose state is the 13 kinematic coordinates AND the
// disturbance force: xi = (x [13], f [3]), 16 states, one v_mfma_f64_16x16x4_f64 tile.  The measurement is the kinematic row alone
// (H = [I13 0]); the row's force slots are never an input.  Per instance it keeps xi [16], P [16][16] (symmetric bit for bit), the time
// word t_prev of the row it last saw and a valid bit.  A call with the measured row z [32] and the applied action u [4]:
//   init     no valid state, or time(z) != t_prev + 1: x = (double)z[0:13], f = 0, P = diag(R, force_init_std^2 I3); row[13:16] = 0,
//            row[0:13] stays as measured
//   predict  x- = model(x, clip(u), f), f- = f; A16 = d(x-, f-)/d(x, f) at xi from 16 forward tangents (qm::D1) = [[A, Bf], [0, I]];
//            P- = (A16 P) A16^T + Q,  Q = diag(proc_std^2 (13), force_walk_std^2 (3))
//   update   S = P-[0:13, 0:13] + R = L D L^T (unpivoted), nu = z - x-, K^T = S^-1 P-[0:13, :] by the two triangular solves (16 x 13),
//            xi = xi- + K nu,  G = I - K H,  P = (G P-) G^T + (K R) K^T, the lower triangle mirrored
//   write    row[0:16] = fp32(xi) -- nothing else of the row --, t_prev = time(z)
// Decided on the device, reported in the side row, none an error (the flags of the state estimator, 4.33):
//   bit 0  initialised: no valid state                   bit 1  re-initialised: the time word
//   bit 2  one of the 13 measured coordinates is not finite: the row is untouched, the filter is invalidated
//   bit 3  a pivot of S is not positive and finite, or xi / P has an entry that is not finite: as an initialisation
//   side row  float[8] = {bits(flags), nu^T S^-1 nu, |nu_pos|, |f^|, P00 + P11 + P22, P13,13 + P14,14 + P15,15, smallest pivot,
//             bits(time)}  (an initialisation: 0 for entries 1 .. 3 and 6; bit 2: 0 for entries 1 .. 6)
//
// One launch, one workgroup of ONE wave per instance; the aim is latency.  Every load -- the row's 17 words, u, xi, the lane's four
// entries of P, the two meta words -- is issued before the first use.  Lane (lo, hi) = (lane & 15, lane >> 4) carries tangent lo
// through the model step: column lo of A16.  A 16 x 16 matrix M lives in the MFMA C/D layout, register r of lane (lo, hi) = M[4r + hi][lo]
// (riccati.hip's): as the B operand of v_mfma_f64_16x16x4_f64 it is M, as the A operand M^T, so a chain of four gives X^T Y.  With P
// symmetric bit for bit P A16^T IS (A16 P)^T, term for term in the same order, and likewise P-^T G^T is (G P-)^T: the five 16 x 16 x 16
// products -- A16 P, (A16 P) A16^T, G P-, (G P-) G^T, (K R) K^T -- need no transpose of a result, only the row-major reads of A16 and
// K from a padded LDS tile ([16][17]).  The 13-pivot elimination and the two solves run in registers as 4.33's do: lane l holds
// column l of S and right-hand side l (lanes 0 .. 15: the columns of P-[0:13, :], lane 16: nu), an entry of another lane arrives by
// v_readlane.  Four LDS tiles (A16, P-, K, the mirror), one wave-level fence each; 8.5 KB.  Batched instances take their argument
// block from device memory, pointers through rebase_global, as state_estimator_kernel does; the log's row index is a kernel argument,
// so the blocks of a steady-state episode never change.
#include "after_step.hpp"
#include "wave_reduce.hpp"

typedef double fo_f64x4 __attribute__((ext_vector_type(4)));

constexpr int FO_BLOCK = COVO_WAVE;
constexpr int FO_N = 16;   // states: 13 kinematic, 3 force
constexpr int FO_NX = 13;  // measured
constexpr int FO_LD = 17;  // leading dimension of the LDS tiles (odd: a column read hits 16 banks)

__device__ __forceinline__ bool fo_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)
__device__ __forceinline__ void fo_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// acc + X^T Y for X, Y in the C/D layout
__device__ __forceinline__ fo_f64x4 fo_mfma4(fo_f64x4 acc, const fo_f64x4 &X, const fo_f64x4 &Y)
{
#pragma unroll
    for (int g = 0; g < 4; ++g) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[g], Y[g], acc, 0, 0, 0);
    return acc;
}

template <bool BATCHED>
__global__ __launch_bounds__(FO_BLOCK) void force_observer_kernel(const ObsDesc D_, const ObsDesc *__restrict__ batch, const int fresh,
                                                                  const int log_index)
{
    __shared__ double sA[FO_N][FO_LD], sM[FO_N][FO_LD], sK[FO_N][FO_LD], sP[FO_N][FO_LD];
    ObsDesc Db;
    if (BATCHED) {
        Db = batch[blockIdx.x];
        Db.state = rebase_global(D_.state, Db.state);
        Db.u = rebase_global(D_.u, Db.u);
        Db.xi = rebase_global(D_.xi, Db.xi);
        Db.P = rebase_global(D_.P, Db.P);
        Db.meta = rebase_global(D_.meta, Db.meta);
        Db.row_out = rebase_global(D_.row_out, Db.row_out);
        Db.log = rebase_global(D_.log, Db.log);
    }
    const ObsDesc &D = BATCHED ? Db : D_;
    const int lane = threadIdx.x, lo = lane & 15, hi = lane >> 4;
    const int c13 = lo < FO_NX ? lo : FO_NX - 1;  // the lane's column of S

    // ---- every load
    float *__restrict__ st = D.state;
    float zf[FO_NX], ff[3], uf[4];
#pragma unroll
    for (int c = 0; c < FO_NX; ++c) zf[c] = st[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) ff[c] = st[ST_FDIST + c];  // (for the log alone: the filter never sees them)
    const int t_z = reinterpret_cast<const int *>(st)[ST_TIME];
#pragma unroll
    for (int c = 0; c < 4; ++c) uf[c] = D.u[c];
    double x[FO_N];
#pragma unroll
    for (int c = 0; c < FO_N; ++c) x[c] = D.xi[c];
    fo_f64x4 P;
#pragma unroll
    for (int r = 0; r < 4; ++r) P[r] = D.P[(4 * r + hi) * FO_N + lo];
    const int valid = fresh ? 0 : D.meta[0];
    const int t_prev = D.meta[1];

    double z[FO_NX];
    bool zfin = true;
#pragma unroll
    for (int c = 0; c < FO_NX; ++c) {
        z[c] = (double)zf[c];
        zfin = zfin && fo_finite(z[c]);
    }
    const bool jump = valid != 0 && t_z != t_prev + 1;
    const bool run = zfin && valid != 0 && !jump;  // (wave-uniform)
    // the diagonals at the lane's own indices: column lo, and the columns 4r + hi of its four registers
    const double R_lo = lo < 3 ? D.R[0] : (lo < 6 ? D.R[1] : (lo < 10 ? D.R[2] : (lo < FO_NX ? D.R[3] : 0.0)));
    const double Q_lo = lo < 3 ? D.Q[0] : (lo < 6 ? D.Q[1] : (lo < 10 ? D.Q[2] : (lo < FO_NX ? D.Q[3] : D.qf)));
    const double P0_lo = lo < FO_NX ? R_lo : D.pf;
    double z_lo = 0.0;
#pragma unroll
    for (int c = 0; c < FO_NX; ++c) z_lo = lo == c ? z[c] : z_lo;

    bool ok = run;
    double xi_new = z_lo, nis = 0.0, innov = 0.0, dmin = 0.0;  // (lanes 0 .. 15: entry lo of xi)
    fo_f64x4 Pn;
#pragma unroll
    for (int r = 0; r < 4; ++r) Pn[r] = (4 * r + hi == lo) ? P0_lo : 0.0;
    if (run) {
        // ---- predict: the model step on tangent lo
        qm::State<qm::D1> s;
        s.px = qm::D1{x[0], lo == 0 ? 1.0 : 0.0};
        s.py = qm::D1{x[1], lo == 1 ? 1.0 : 0.0};
        s.pz = qm::D1{x[2], lo == 2 ? 1.0 : 0.0};
        s.vx = qm::D1{x[3], lo == 3 ? 1.0 : 0.0};
        s.vy = qm::D1{x[4], lo == 4 ? 1.0 : 0.0};
        s.vz = qm::D1{x[5], lo == 5 ? 1.0 : 0.0};
        s.qx = qm::D1{x[6], lo == 6 ? 1.0 : 0.0};
        s.qy = qm::D1{x[7], lo == 7 ? 1.0 : 0.0};
        s.qz = qm::D1{x[8], lo == 8 ? 1.0 : 0.0};
        s.qw = qm::D1{x[9], lo == 9 ? 1.0 : 0.0};
        s.ox = qm::D1{x[10], lo == 10 ? 1.0 : 0.0};
        s.oy = qm::D1{x[11], lo == 11 ? 1.0 : 0.0};
        s.oz = qm::D1{x[12], lo == 12 ? 1.0 : 0.0};
        const qm::D1 f0{x[13], lo == 13 ? 1.0 : 0.0}, f1{x[14], lo == 14 ? 1.0 : 0.0}, f2{x[15], lo == 15 ? 1.0 : 0.0};
        const qm::D1 a0{qm::clip11_((double)uf[0]), 0.0}, a1{qm::clip11_((double)uf[1]), 0.0}, a2{qm::clip11_((double)uf[2]), 0.0},
            a3{qm::clip11_((double)uf[3]), 0.0};
        qm::dyn_step<qm::D1, double, true, qm::D1>(s, a0, a1, a2, a3, D.c, f0, f1, f2);
        const double xm[FO_NX] = {s.px.v, s.py.v, s.pz.v, s.vx.v, s.vy.v, s.vz.v, s.qx.v, s.qy.v, s.qz.v, s.qw.v, s.ox.v, s.oy.v, s.oz.v};
        const double a[FO_NX] = {s.px.a, s.py.a, s.pz.a, s.vx.a, s.vy.a, s.vz.a, s.qx.a, s.qy.a, s.qz.a, s.qw.a, s.ox.a, s.oy.a, s.oz.a};
        // a[i] (tangent lo) = A16[i][lo]; rows 13 .. 15 of A16 are [0 I].  At = A16^T in the C/D layout: register r = A16[lo][4r + hi]
        if (hi == 0) {
#pragma unroll
            for (int i = 0; i < FO_NX; ++i) sA[i][lo] = a[i];
#pragma unroll
            for (int i = FO_NX; i < FO_N; ++i) sA[i][lo] = lo == i ? 1.0 : 0.0;
        }
        fo_wave_sync();
        fo_f64x4 At;
#pragma unroll
        for (int r = 0; r < 4; ++r) At[r] = sA[lo][4 * r + hi];
        const fo_f64x4 zero = {0.0, 0.0, 0.0, 0.0};
        const fo_f64x4 T1t = fo_mfma4(zero, P, At);  // P A16^T = (A16 P)^T
        fo_f64x4 Pm;
#pragma unroll
        for (int r = 0; r < 4; ++r) Pm[r] = (4 * r + hi == lo) ? Q_lo : 0.0;
        Pm = fo_mfma4(Pm, T1t, At);  // (A16 P) A16^T + Q
#pragma unroll
        for (int r = 0; r < 4; ++r) sM[4 * r + hi][lo] = Pm[r];
        fo_wave_sync();
        // ---- S = P-[0:13, 0:13] + R = L D L^T by symmetric elimination: sc[i] (lane l < 13) = S[i][l]; after step k lane l > k holds
        // L[l][k] in lk[k].  The right-hand sides: lane l < 16 column l of P-[0:13, :], lane 16 nu
        double sc[FO_NX], lk[FO_NX], dk[FO_NX], nu[FO_NX], y[FO_NX];
#pragma unroll
        for (int i = 0; i < FO_NX; ++i) {
            sc[i] = sM[i][c13] + (c13 == i ? R_lo : 0.0);
            nu[i] = z[i] - xm[i];
            y[i] = lane == FO_N ? nu[i] : sM[i][lo];
        }
        dmin = __builtin_inf();
#pragma unroll
        for (int k = 0; k < FO_NX; ++k) {
            const double d = wr::bcast_lane(sc[k], k);
            ok = ok && d > 0.0 && fo_finite(d);
            dmin = fmin(dmin, d);
            dk[k] = qm::rcp64_(d);
            const double f = sc[k] * dk[k];  // S[k][l] / d = L[l][k] (by symmetry the lane's own entry)
            lk[k] = f;
#pragma unroll
            for (int i = k + 1; i < FO_NX; ++i) sc[i] = fma(-wr::bcast_lane(sc[i], k), f, sc[i]);
        }
#pragma unroll
        for (int i = 1; i < FO_NX; ++i) {
#pragma unroll
            for (int k = 0; k < i; ++k) y[i] = fma(-wr::bcast_lane(lk[k], i), y[k], y[i]);
        }
#pragma unroll
        for (int i = 0; i < FO_NX; ++i) y[i] *= dk[i];
#pragma unroll
        for (int i = FO_NX - 2; i >= 0; --i) {
#pragma unroll
            for (int k = i + 1; k < FO_NX; ++k) y[i] = fma(-wr::bcast_lane(lk[i], k), y[k], y[i]);
        }
        // lane l < 16: y[i] = (S^-1 P-[0:13, :])[i][l] = K[l][i]; lane 16: S^-1 nu
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < FO_NX; ++i) dot = fma(y[i], nu[i], dot);
        nis = wr::bcast_lane(dot, FO_N);
        innov = sqrt(fma(nu[2], nu[2], fma(nu[1], nu[1], nu[0] * nu[0])));
        double xm_lo = x[FO_NX];  // (f- = f)
        xm_lo = lo == FO_NX + 1 ? x[FO_NX + 1] : (lo == FO_NX + 2 ? x[FO_NX + 2] : xm_lo);
#pragma unroll
        for (int c = 0; c < FO_NX; ++c) xm_lo = lo == c ? xm[c] : xm_lo;
        xi_new = xm_lo + dot;
        // ---- Joseph.  K's rows (padded with H's three zero columns) through LDS: Kt = K^T, Gt = (I - K H)^T, KRt = (K R)^T
        if (lane < FO_N) {
#pragma unroll
            for (int i = 0; i < FO_NX; ++i) sK[lane][i] = y[i];
#pragma unroll
            for (int i = FO_NX; i < FO_N; ++i) sK[lane][i] = 0.0;
        }
        fo_wave_sync();
        fo_f64x4 Kt, Gt, KRt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 4 * r + hi;
            const double R_col = col < 3 ? D.R[0] : (col < 6 ? D.R[1] : (col < 10 ? D.R[2] : (col < FO_NX ? D.R[3] : 0.0)));
            Kt[r] = sK[lo][col];
            Gt[r] = (col == lo ? 1.0 : 0.0) - Kt[r];
            KRt[r] = Kt[r] * R_col;
        }
        const fo_f64x4 T2t = fo_mfma4(zero, Pm, Gt);  // P-^T G^T = (G P-)^T
        Pn = fo_mfma4(zero, T2t, Gt);                 // (G P-) G^T
        Pn = fo_mfma4(Pn, KRt, Kt);                   // + (K R) K^T
        // the lower triangle mirrored
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[4 * r + hi][lo] = Pn[r];
        fo_wave_sync();
        bool fin = lane >= FO_N || fo_finite(xi_new);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Pn[r] = lo <= 4 * r + hi ? Pn[r] : sP[lo][4 * r + hi];
            fin = fin && fo_finite(Pn[r]);
        }
        ok = ok && __all(fin ? 1 : 0) != 0;
        if (!ok) {  // (uniform) as an initialisation
            xi_new = z_lo;
#pragma unroll
            for (int r = 0; r < 4; ++r) Pn[r] = (4 * r + hi == lo) ? P0_lo : 0.0;
            nis = innov = dmin = 0.0;
        }
    }
    const int flags = !zfin ? 4 : (valid == 0 ? 1 : (jump ? 2 : (ok ? 0 : 8)));
    const bool wrote = zfin && ok;  // the row receives the estimate (otherwise, unless bit 2, its force slots receive 0)
    if (!wrote) xi_new = lo < FO_NX ? z_lo : 0.0;
    // the row's statistics: f^ lives in lanes 13 .. 15, P[i][i] in register i >> 2 of lane (lo, hi) = (i, i & 3)
    const double f0 = wr::bcast_lane(xi_new, 13), f1 = wr::bcast_lane(xi_new, 14), f2 = wr::bcast_lane(xi_new, 15);
    const double fnorm = sqrt(fma(f2, f2, fma(f1, f1, f0 * f0)));
    const double tr_pos = wr::bcast_lane(Pn[0], 0) + wr::bcast_lane(Pn[0], 17) + wr::bcast_lane(Pn[0], 34);
    const double tr_f = wr::bcast_lane(Pn[3], 29) + wr::bcast_lane(Pn[3], 46) + wr::bcast_lane(Pn[3], 63);

    // ---- stores
    const float x32 = (float)xi_new;
    if (zfin) {
        if (lane < FO_N) {
            D.xi[lane] = xi_new;
            if (wrote || lane >= FO_NX) st[lane] = x32;  // (not updated: the force slots alone, 0)
        } else if (lane == FO_N) {
            D.meta[0] = 1;
            D.meta[1] = t_z;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) D.P[(4 * r + hi) * FO_N + lo] = Pn[r];
    } else if (lane == FO_N) {
        D.meta[0] = 0;
    }
    float w8 = 0.0f;
    if (lane < COVO_OBS_FLOATS) {
        const bool stats = zfin;
        w8 = lane == 0   ? __int_as_float(flags)
             : lane == 1 ? (float)nis
             : lane == 2 ? (float)innov
             : lane == 3 ? (stats ? (float)fnorm : 0.0f)
             : lane == 4 ? (stats ? (float)tr_pos : 0.0f)
             : lane == 5 ? (stats ? (float)tr_f : 0.0f)
             : lane == 6 ? (float)dmin
                         : __int_as_float(t_z);
        if (D_.row_out != nullptr) D.row_out[lane] = w8;
    }
    if (D_.log != nullptr && log_index >= 0) {
        float *lg = D.log + (size_t)log_index * COVO_OBS_LOG_FLOATS;
        if (lane < FO_N) {
            float zl = lane == FO_NX ? ff[0] : (lane == FO_NX + 1 ? ff[1] : ff[2]);  // (the true force: the plant's, for the reader)
#pragma unroll
            for (int c = 0; c < FO_NX; ++c) zl = lane == c ? zf[c] : zl;
            lg[lane] = zl;
            lg[FO_N + lane] = zfin ? x32 : zl;
        }
        if (lane < COVO_OBS_FLOATS) lg[2 * FO_N + lane] = w8;
    }
}

// ---- host
int observer_fill_model(ObsDesc &d, const covo_env_params &p, const double *obs_std, const double *proc_std, double force_walk_std,
                        double force_init_std, const char *what)
{
    const double inf = __builtin_inf();
    for (int g = 0; g < 4; ++g) {
        REQUIRE(obs_std[g] > 0.0 && obs_std[g] < inf, "%s: obs_std[%d]=%g is not a positive finite number", what, g, obs_std[g]);
        REQUIRE(proc_std[g] >= 0.0 && proc_std[g] < inf, "%s: proc_std[%d]=%g is not a finite number >= 0", what, g, proc_std[g]);
        d.R[g] = obs_std[g] * obs_std[g];
        d.Q[g] = proc_std[g] * proc_std[g];
    }
    REQUIRE(force_walk_std >= 0.0 && force_walk_std < inf, "%s: force_walk_std=%g is not a finite number >= 0", what, force_walk_std);
    REQUIRE(force_init_std >= 0.0 && force_init_std < inf, "%s: force_init_std=%g is not a finite number >= 0", what, force_init_std);
    d.qf = force_walk_std * force_walk_std;
    d.pf = force_init_std * force_init_std;
    d.c = make_consts<double>(p);
    return 0;
}

int launch_force_observer(covo_ctx *h, const ObsDesc *d, int n_inst, bool batched, bool primitive, int fresh, int log_index, hipStream_t s)
{
    if (n_inst < 1 || n_inst > COVO_MAX_ENVS) {
        covo_set_error("force observer: n_inst=%d outside (0, %d]", n_inst, COVO_MAX_ENVS);
        return COVO_E_BADARG;
    }
    if (!batched) {
        hipLaunchKernelGGL(force_observer_kernel<false>, dim3(1), dim3(FO_BLOCK), 0, s, d[0], (const ObsDesc *)nullptr, fresh, log_index);
    } else {
        ArgBlockCache &c = primitive ? after_state(h)->obs_primitive : after_state(h)->obs;
        if (int rc = c.sync_upload(d, (size_t)n_inst * sizeof(ObsDesc), sizeof(ObsDesc), s)) return rc;
        hipLaunchKernelGGL(force_observer_kernel<true>, dim3(n_inst), dim3(FO_BLOCK), 0, s, d[0], (const ObsDesc *)c.dev, fresh, log_index);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int covo_force_observer_step(covo_ctx *h, float *states, const float *a_mean, const covo_env_params *params, int n_inst, bool batched,
                             int log_index, hipStream_t s)
{
    if (!covo_force_observer_on(h)) return 0;
    static thread_local ObsDesc d[COVO_MAX_ENVS];
    std::memset(d, 0, (size_t)n_inst * sizeof(ObsDesc));
    for (int e = 0; e < n_inst; ++e) {
        if (int rc = observer_fill_model(d[e], params[e], h->obs_obs_std, h->obs_proc_std, h->obs_walk_std, h->obs_init_std,
                                         "covo_set_step_force_observer"))
            return rc;
        d[e].state = states + (size_t)e * COVO_STATE_FLOATS;
        d[e].u = a_mean + (size_t)e * COVO_NA;
        d[e].xi = h->obs_xi + (size_t)e * COVO_OBS_STATE_DOUBLES;
        d[e].P = h->obs_P + (size_t)e * FO_N * FO_N;
        d[e].meta = h->obs_meta + (size_t)e * COVO_OBS_META_INTS;
        d[e].row_out = h->obs_rows + (size_t)e * COVO_OBS_FLOATS;
        d[e].log = h->obs_log ? h->obs_log + (size_t)e * h->obs_log_stride * COVO_OBS_LOG_FLOATS : nullptr;
    }
    const int fresh = h->obs_fresh;
    h->obs_fresh = 0;
    return launch_force_observer(h, d, n_inst, batched, false, fresh, log_index, s);
}
