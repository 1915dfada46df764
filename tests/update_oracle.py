"""A plain fp64 reference of the weighted update (numpy only; not collected by pytest), and the crafted inputs of its tests.

The update (covo.py:266-275, mppi.py:109-125):  w_n = exp(-(c_n - min c) / lam) / sum,  a_mean' = gamma sum_n w_n a_n + (1 - gamma) a_mean,
MPPI with gamma_sigma != 0:  a_cov'[t] = gamma_sigma sum_n w_n (a_n[t] - a_mean'[t]) (a_n[t] - a_mean'[t])^T + (1 - gamma_sigma) a_cov[t].
Every function takes the device's own fp32 arrays (the step's costs and actions), widens them to fp64 and evaluates the formulas as
written: the cost error of an fp64 rollout is out of the picture, what remains is the error of the update's own fp32 sums, and the
bar is the project's 1e-5 absolute.  lambda reaches the kernels as the float 1 / lam: the reference multiplies by the
same float (as tests/test_gpu_diag.py::_reference).

Used by tests/test_update_oracle.py (CPU: against oracle/ref_np.py), tests/test_gpu_update_edges.py (crafted inputs through the C ABI)
and tests/test_gpu_update_paths.py (the mean of real steps on every path).
"""
import numpy as np

H, DU, NA = 32, 4, 128
PARTIAL_FLOATS = 132                 # {m, s, v[128], pad[2]}
COV_FLOATS = 320                     # the 10 second moments i <= j of every step
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]  # their order in a record (csrc/softmax_stage1.hpp: cov_pair)
BAR = 1e-5                           # absolute, on a_mean in [-1, 1] and on a_cov


def inv_lam64(lam):
    """1 / lam as the kernels receive it: the fp32 quotient, widened."""
    return np.float64(np.float32(1.0) / np.float32(lam))


def weights_f32(cost_f32, lam):
    """The kernels' weight expression expf((m - c) * inv_lam) emulated in numpy fp32 (every operation rounded to fp32)."""
    c = np.asarray(cost_f32, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(lam)
    with np.errstate(under="ignore"):
        return np.exp(((c.min() - c) * inv).astype(np.float32)).astype(np.float32)


def n_live(cost_f32, lam):
    """Samples whose fp32 weight is > 0: the ones the update's kernels read the actions of."""
    return int((weights_f32(cost_f32, lam) > 0).sum())


def _weights(cost, lam):
    c = np.asarray(cost, dtype=np.float64)
    with np.errstate(under="ignore"):
        return c.min(), np.exp(-(c - c.min()) * inv_lam64(lam))


def mean64(cost, a, lam, gamma, a_mean_old):
    """cost [N], a [N, 32, 4], a_mean_old [32, 4] -> (new mean [32, 4], normalised weights [N]), fp64."""
    _, e = _weights(cost, lam)
    w = e / e.sum()
    wmean = np.tensordot(w, np.asarray(a, dtype=np.float64), axes=1)
    return wmean * np.float64(gamma) + np.asarray(a_mean_old, dtype=np.float64) * (1.0 - np.float64(gamma)), w


def cov64(weights, a, mean_new, a_cov_old, gamma_sigma):
    """mppi.py:119-125: the weighted covariance of every step's four action components about the NEW mean, blended.
    a [N, 32, 4], mean_new [32, 4], a_cov_old [32, 4, 4] -> [32, 4, 4]."""
    d = (np.asarray(a, dtype=np.float64) - np.asarray(mean_new, dtype=np.float64)[None]).transpose(1, 2, 0)  # [32, 4, N]
    C = (d * np.asarray(weights, dtype=np.float64)) @ d.transpose(0, 2, 1)  # sum_n w_n d_n[t] d_n[t]^T for every step t
    return C * np.float64(gamma_sigma) + np.asarray(a_cov_old, dtype=np.float64) * (1.0 - np.float64(gamma_sigma))


def ess64(weights):
    w = np.asarray(weights, dtype=np.float64)
    return float(w.sum() ** 2 / (w * w).sum())


def record64(cost, a, lam, mu=None):
    """The online-softmax record of one shard: {m = min c, s = sum w, v[128] = sum w a} with w = exp(-(c - m) / lam), unnormalised.
    mu [32, 4] given: also S2 [32, 4, 4] = sum_n w_n d_n d_n^T of every step, d = a - mu, and s2 [320], its 10 entries i <= j per step
    in the record's order.  An empty shard (N = 0): m = +inf, s = 0, v = 0."""
    c = np.asarray(cost, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64).reshape(len(c), H, DU)
    if len(c) == 0:
        rec = dict(m=np.float64(np.inf), s=np.float64(0.0), v=np.zeros(NA))
        w = np.zeros(0)
    else:
        m, w = _weights(c, lam)
        rec = dict(m=m, s=w.sum(), v=w @ a.reshape(len(c), NA))
    if mu is not None:
        d = a - np.asarray(mu, dtype=np.float64)[None]
        rec["S2"] = np.einsum("n,nti,ntj->tij", w, d, d)
        rec["s2"] = pack_pairs(rec["S2"])
    return rec


def pack_pairs(S2):
    """[32, 4, 4] symmetric -> the record's [320]: entries (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3) per step."""
    return np.stack([S2[:, i, j] for i, j in PAIRS], axis=1).reshape(-1)


def unpack_pairs(s2):
    s2 = np.asarray(s2, dtype=np.float64).reshape(H, 10)
    S2 = np.zeros((H, DU, DU))
    for k, (i, j) in enumerate(PAIRS):
        S2[:, i, j] = S2[:, j, i] = s2[:, k]
    return S2


def record_row(rec, floats=PARTIAL_FLOATS):
    """A record64 as one fp32 row of `floats` floats: {m, s, v[128], 0, 0} and, where the record has them and the row the room, the
    320 second moments behind; everything after stays 0 (a rank record's position sums)."""
    row = np.zeros(floats, dtype=np.float32)
    row[0], row[1], row[2:2 + NA] = rec["m"], rec["s"], rec["v"]
    if "s2" in rec and floats >= PARTIAL_FLOATS + COV_FLOATS:
        row[PARTIAL_FLOATS:PARTIAL_FLOATS + COV_FLOATS] = rec["s2"]
    return row


def empty_row(floats=PARTIAL_FLOATS, garbage=None):
    """The record of a shard without samples: m = +inf, s = 0, v = 0 -- or `garbage` in v (and the second moments), which a merge
    must not let through."""
    row = np.zeros(floats, dtype=np.float32)
    row[0] = np.inf
    if garbage is not None:
        row[2:2 + NA] = garbage
        if floats >= PARTIAL_FLOATS + COV_FLOATS:
            row[PARTIAL_FLOATS:PARTIAL_FLOATS + COV_FLOATS] = garbage
    return row


def merge64(records, lam, gamma=None, a_mean_old=None, a_cov_old=None, gamma_sigma=None):
    """The online-softmax rule over G records [G, stride >= 130] in fp64: m = min_g m_g, scale_g = exp(-(m_g - m) / lam),
    s = sum_g s_g scale_g, v = sum_g v_g scale_g; a record with s_g = 0 contributes nothing, whatever its other floats hold.
    Returns {m, s, v, scale}; with gamma and a_mean_old [32, 4] also `mean` = gamma v / s + (1 - gamma) a_mean_old; with a_cov_old and
    gamma_sigma (records of stride >= 452 with second moments about a_mean_old) also `cov` [32, 4, 4], from
    sum w (d - e)(d - e)^T = S2 - m1 e^T - e m1^T + e e^T with d = a - mu, m1 = sum w d, e = mean' - mu (sum w = 1)."""
    r = np.asarray(records, dtype=np.float64)
    mg, sg = r[:, 0], r[:, 1]
    m = mg.min()
    live = sg > 0
    with np.errstate(under="ignore", invalid="ignore"):
        scale = np.where(live, np.exp(-(mg - m) * inv_lam64(lam)), 0.0)
    s = (sg[live] * scale[live]).sum()
    v = scale[live] @ r[live, 2:2 + NA]
    out = dict(m=m, s=s, v=v, scale=scale)
    if a_mean_old is not None:
        mu = np.asarray(a_mean_old, dtype=np.float64).reshape(H, DU)
        wmean = (v / s).reshape(H, DU)
        out["mean"] = wmean * np.float64(gamma) + mu * (1.0 - np.float64(gamma))
        if a_cov_old is not None:
            S2 = unpack_pairs(scale[live] @ r[live, PARTIAL_FLOATS:PARTIAL_FLOATS + COV_FLOATS]) / s
            m1, e = wmean - mu, out["mean"] - mu
            C = S2 - m1[:, :, None] * e[:, None, :] - e[:, :, None] * m1[:, None, :] + e[:, :, None] * e[:, None, :]
            out["cov"] = C * np.float64(gamma_sigma) + np.asarray(a_cov_old, dtype=np.float64) * (1.0 - np.float64(gamma_sigma))
    return out


def stripes(a_hn4):
    """The device layout [H][N][4] (numpy, or a torch tensor on any device) -> [N, H, 4] numpy."""
    if hasattr(a_hn4, "detach"):
        a_hn4 = a_hn4.detach().cpu().numpy()
    return np.ascontiguousarray(np.transpose(np.asarray(a_hn4), (1, 0, 2)))


def from_stripes(a_nh4):
    """[N, H, 4] -> the device layout [H][N][4], fp32 numpy (test_gpu_parity.py::to_stripes puts the same on the device)."""
    return np.ascontiguousarray(np.transpose(np.asarray(a_nh4), (1, 0, 2)), dtype=np.float32)


# ------------------------------------------------------------------------------------------ crafted inputs
# 65 600: 1 025 full groups over the capped grid's 1 024 waves (the smallest shape whose waves stride); 65 570: the same with the
# strided group partial (34 samples)
EDGE_SIZES = (1, 63, 64, 65, 255, 257, 1025, 65600, 65570)
EDGE_LAMS = (0.01, 1.0, 1e4)
PATTERNS = ("equal", "winner", "winner_last", "tied", "offset", "gauss", "lanes")
LANE_COUNTS = (0, 1, 2, 7, 8, 9, 63, 64)
MERGE_GS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024)
RANK_GS = (1, 8, 65, 257)
MERGE_VARIANTS = ("as_is", "empty", "empty_garbage", "empty_stale", "underflow", "equal_m")


def actions(N, seed=0):
    """(a [N, 32, 4], a_mean_old [32, 4], a_cov_old [32, 4, 4]) fp32: clipped samples as a step draws them."""
    rng = np.random.default_rng(1000 + seed)
    a = np.clip(0.6 * rng.normal(size=(N, H, DU)), -1, 1).astype(np.float32)
    mean = (0.1 * rng.normal(size=(H, DU))).astype(np.float32)
    B = rng.normal(size=(H, DU, DU))
    cov = (0.05 * B @ B.transpose(0, 2, 1) + 0.1 * np.eye(DU)).astype(np.float32)
    return a, mean, cov


def tied_positions(N):
    """Two sample indices in different 64-sample waves where N > 64, in different stage-1 workgroups (256 samples each; the capped
    grid wraps after 1 024 waves) where N > 256."""
    groups = (N + 63) // 64
    g = groups - 1 if groups <= 1024 else groups // 2
    return min(3, N - 1), min(64 * g + 5, N - 1) if N > 1 else 0


def winner_index(pattern, N):
    return N - 1 if pattern == "winner_last" else (N * 5) // 11


def lane_plan(N, rng):
    """Per 64-sample group a live count from LANE_COUNTS (capped by the group's size), at random lanes -> bool [N].  Every count is
    used when there are at least 8 groups; some group is live."""
    groups = (N + 63) // 64
    counts = np.array([LANE_COUNTS[i % 8] for i in rng.permutation(groups)]) if groups >= 8 else rng.choice(LANE_COUNTS, groups)
    live = np.zeros(groups * 64, dtype=bool)
    for g, k in enumerate(counts):
        size = min(64, N - 64 * g)
        live[64 * g + rng.permutation(size)[:min(k, size)]] = True
    live = live[:N]
    if not live.any():
        live[rng.integers(N)] = True
    return live


def cost_pattern(pattern, N, lam, seed=0):
    """The fp32 costs [N] of one crafted case (the properties the GPU tests rely on are asserted in tests/test_update_oracle.py):
      equal        all costs equal: every weight is 1
      winner       one sample 50 below the rest (at lam = 0.01 every other fp32 weight is exactly 0)
      winner_last  the same at n = N - 1, in the last (partial) group
      tied         two exactly tied minima in different waves / workgroups (tied_positions)
      offset       1e6 + 0.0625 k: a large offset with fp32-exact differences
      gauss        Gaussian 5 +- 3
      lanes        per 64-group a live lane count from LANE_COUNTS: costs within 0.5 lam of the minimum, or 200 lam (and more) above"""
    rng = np.random.default_rng(7919 * PATTERNS.index(pattern) + 31 * N + seed)
    gauss = (5.0 + 3.0 * rng.normal(size=N)).astype(np.float32)
    if pattern == "equal":
        return np.full(N, 5.25, dtype=np.float32)
    if pattern in ("winner", "winner_last"):
        c = gauss.copy()
        i = winner_index(pattern, N)
        c[i] = np.float32(np.delete(c, i).min() - 50.0) if N > 1 else c[i]
        return c
    if pattern == "tied":
        c = gauss.copy()
        i, j = tied_positions(N)
        c[i] = c[j] = np.float32(c.min() - 0.25)
        return c
    if pattern == "offset":
        return (np.float64(1e6) + 0.0625 * rng.integers(0, 4096, size=N)).astype(np.float32)
    if pattern == "gauss":
        return gauss
    if pattern == "lanes":
        live = lane_plan(N, rng)
        lam = np.float64(lam)
        c = np.where(live, 5.0 + 0.5 * lam * rng.random(N), 5.0 + lam * (200.0 + 50.0 * rng.random(N)))
        c[np.flatnonzero(live)[rng.integers(live.sum())]] = 5.0  # the minimum itself
        return c.astype(np.float32)
    raise ValueError(pattern)


def lanes_live_mask(N, seed=0):
    """The live mask cost_pattern("lanes", N, ., seed) was built from (the same generator state)."""
    rng = np.random.default_rng(7919 * PATTERNS.index("lanes") + 31 * N + seed)
    rng.normal(size=N)
    return lane_plan(N, rng)


def shard_records(G, lam, variant, n=16, seed=0, floats=PARTIAL_FLOATS, with_cov=False):
    """G records as fp32 rows [G, floats], built with record64 from random shards of n samples each (costs 5 + 3 lam normal, so the
    records' scales spread over some e-folds at every lam), then rounded to fp32; (rows, mu): mu [32, 4] fp32 is the mean the second
    moments (with_cov) are about.  Variants:
      as_is          as built
      empty          every third record (g % 3 == 1) empty: m = +inf, s = 0, v = 0
      empty_garbage  the same with 1e30 in the empty records' v (and second moments)
      empty_stale    the same with, besides, a stale finite minimum (that of the record before) in the empty records' m: s = 0 alone
                     says that a record is empty
      underflow      the records' minima 0.5 apart (shuffled): at lam = 0.01 the scale of the nearest record is exp(-50) = 2e-22, that
                     of the next one a denormal (or 0) and that of every other one underflows to exactly 0 in fp32
      equal_m        all m_g equal"""
    rng = np.random.default_rng(4242 + seed)
    mu = (0.1 * rng.normal(size=(H, DU))).astype(np.float32)
    order = rng.permutation(G)
    rows = np.zeros((G, floats), dtype=np.float32)
    for g in range(G):
        c = (5.0 + 3.0 * lam * rng.normal(size=n)).astype(np.float32)
        a = np.clip(0.6 * rng.normal(size=(n, H, DU)), -1, 1).astype(np.float32)
        if variant == "underflow":
            c = (c - c.min() + np.float32(5.0 + 0.5 * order[g])).astype(np.float32)
            c[np.argmin(c)] = np.float32(5.0 + 0.5 * order[g])
        if variant == "equal_m":
            c[rng.integers(n)] = np.float32(5.0 - 4.0 * 3.0 * lam)
        if variant in ("empty", "empty_garbage", "empty_stale") and g % 3 == 1:
            rows[g] = empty_row(floats, garbage=None if variant == "empty" else np.float32(1e30))
            if variant == "empty_stale":
                rows[g, 0] = rows[g - 1, 0]
        else:
            rows[g] = record_row(record64(c, a, lam, mu if with_cov else None), floats)
    return rows, mu


def pad_rows(rows, G_to):
    """The same records followed by empty ones (m = +inf, s = 0, v = 0) up to G_to."""
    pad = np.stack([empty_row(rows.shape[1])] * (G_to - len(rows))) if G_to > len(rows) else np.zeros((0, rows.shape[1]), np.float32)
    return np.concatenate([rows, pad.astype(np.float32)], axis=0)


# ------------------------------------------------------------------------------------------ the update of a real step
def _np(x):
    """numpy of a numpy array or of a torch tensor on any device."""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def regime(live, N):
    """Which of the three live-sample regimes a step ran in: "few" (n_live <= 8: the update copies a handful of samples), "all"
    (n_live == N: whole waves), "some" (in between: partly live waves and sub-groups)."""
    return "few" if live <= 8 else "all" if live == N else "some"


def check_update(core_or_views, a_mean_before, gamma_mean, lam, a_mean_new, a_cov_old=None, gamma_sigma=None, a_cov_new=None,
                 where="", bar=BAR, shifted=False):
    """The update of a step that has run, against mean64 (and cov64) on the step's OWN fp32 costs and actions, read back from the
    device: core_or_views is a SamplingCore (its .cost [N] and .a [32][N][4]) or the pair (cost, a) of an instance's views.
    a_mean_before [32, 4] (and MPPI's a_cov_old [32, 4, 4]) are the control parameters the step was called with: the step shifts
    them (covo.py:201-203, mppi.py:43-49) and so does the reference (shifted=True: they are the shifted ones already, as the
    stand-alone covo_softmax_update takes them).  Asserts <= 1e-5 absolute on the mean (and the covariance),
    prints the errors, the fp64 ESS and n_live (samples whose fp32 weight is > 0) and returns them."""
    from oracle import ref_np as R
    cost, a = (core_or_views.cost, core_or_views.a) if hasattr(core_or_views, "cost") else core_or_views
    cost, a = _np(cost).astype(np.float32), stripes(a).astype(np.float64)
    mu = _np(a_mean_before).astype(np.float64).reshape(H, DU)
    mu = mu if shifted else R.shift_mean(mu)
    ref, w = mean64(cost, a, lam, gamma_mean, mu)
    out = dict(err=float(np.abs(_np(a_mean_new).reshape(H, DU) - ref).max()), ess=ess64(w), n_live=n_live(cost, lam), N=len(cost),
               err_cov=None)
    if a_cov_new is not None:
        cov = _np(a_cov_old).astype(np.float64).reshape(H, DU, DU)
        cov = cov if shifted else np.concatenate([cov[1:], cov[-1:]], axis=0)
        out["err_cov"] = float(np.abs(_np(a_cov_new).reshape(H, DU, DU) - cov64(w, a, ref, cov, gamma_sigma)).max())
    print(f"  update vs fp64 on the step's own costs {where}: N {out['N']} lam {float(lam):g} err {out['err']:.2e}" +
          (f" cov err {out['err_cov']:.2e}" if out["err_cov"] is not None else "") +
          f" ess {out['ess']:.2f} n_live {out['n_live']} ({regime(out['n_live'], out['N'])})")
    assert out["err"] <= bar, (where, out)
    assert out["err_cov"] is None or out["err_cov"] <= bar, (where, out)
    return out


def lam_for_live(cost_f32, k):
    """A temperature at which about k samples of these costs keep an fp32 weight > 0: the k-th smallest cost lies 105 lam above the
    minimum (expf underflows to exactly 0 below -103.98)."""
    c = np.sort(np.asarray(cost_f32, dtype=np.float64))
    k = min(int(k), len(c) - 1)
    return float((c[k] - c[0]) / 105.0)
