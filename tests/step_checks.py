"""What the absolute checks of one ALM iteration share (test_step_checks_cpu.py, test_hip_step_variants.py; plain numpy, TEST INFRASTRUCTURE):

``edge_state``     a state on which the cone projection takes every branch, sits exactly on both boundaries and has a zero pre-image;
``check_one_step`` the state after one iteration against the fp64 oracle, entry by entry, with phi taken from the side under test;
``SCENARIOS``      the flag combinations of ``dots_step`` that select the direct solver's kernel variants, as drivers that work on
                   anything with ``DeviceProblem``'s calls (the GPU, or ``OracleDevice`` below on the CPU)."""
import os

import numpy as np

from conftest import GOLDEN_DIR, load_oracle

O = load_oracle()
STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
DUAL = ("mu", "E", "beta_fst", "beta_mid", "beta_end")
FP_TOL = 1e-12      # fp64 element-wise kernels vs numpy: summation order only (test_hip_phases.py)
PHI_TOL = 1e-9      # the solve (test_laplacian_step_a2_a3)
KKT_TOL = 1e-11     # the residuals (test_kkt_objective_norms_a10_a11_a12)
MESHES = ("ops_ico1", "ops_refplane4", "fan")
# pitches 8, 8, 8 (full), 16 (ragged), 32, 64 (matrix cores, full), 128 (matrix cores, ragged); both parities; T = 1: no second interval at all
T_ALL = (1, 6, 7, 8, 31, 63, 64)
T_FEW = (7, 64)     # one small-pitch and one matrix-core T for the scenarios that do not run on all of them
FACTOR = 1.7        # the penalty update of the scenarios with a pending division


def fan_geometry():
    """An open fan: hub 0 of valence 9 (odd, more than two CARRY_BATCH loads), rim vertices 1..10 of valence 2, the two ends of valence 1;
    V = 11, F = 9; positive densities of equal mass."""
    ang = np.deg2rad(33.0) * np.arange(10)
    rad = 1.0 + 0.07 * np.arange(10)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.05 * np.sin(3.0 * ang)], axis=1)
    vertices = np.concatenate([np.zeros((1, 3)), rim])
    triangles = np.array([[0, i, i + 1] for i in range(1, 10)], dtype=np.int32)
    rng = np.random.default_rng(11)
    mu0, mu1 = rng.uniform(0.5, 1.5, 11), rng.uniform(0.5, 1.5, 11)
    return dict(vertices=vertices, triangles=triangles, mu0=mu0 / mu0.sum(), mu1=mu1 / mu1.sum())


def geometry(mesh):
    if mesh == "fan":
        return fan_geometry()
    g = np.load(os.path.join(GOLDEN_DIR, mesh + ".npz"))
    return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])


def make_oracle(T, geom, congestion=0.0):
    """The oracle with the parameters of make_pair (test_hip_phases.py)."""
    s = O.OracleSolver(T, geom, congestion=congestion)
    s.r, s.sz, s.d = 1.7, 2.5, 1.3
    s.norm_d *= 1.3
    s.bnd /= s.r
    return s


def device_params(s):
    return dict(r=s.r, scale_z=s.sz, const_d=s.d, norm_d=s.norm_d, congestion=s.congestion, eps=s.eps, tau=s.tau)


def snapshot(s):
    return {k: getattr(s, k).copy() for k in STATE}


def load(s, state):
    for k in STATE:
        setattr(s, k, np.array(state[k], dtype=np.float64, copy=True))


def valence(s):
    return np.bincount(s.tri.reshape(-1), minlength=s.V)


# ---- the cone projection, restated with the knobs of the deliberate mutations ------------------------------------------------
def cone_preimage(s, drop_last_corner=False):
    """w_fst, w_end, w_mid and the norm of the projection's pre-image (oracle: step_soc_projection).  ``drop_last_corner``: the last
    corner of every odd-valence vertex's list is left out of the norm (a CARRY_BATCH tail that is never added)."""
    w_fst = s.d - s.sz * s.A - s.beta_fst
    w_mid = s.D[None, None, :, :, None] * (O.decouple(s.B, s.sz) - s.beta_mid)
    w_end = s.d + s.sz * s.A - s.beta_end
    per_corner = (w_mid ** 2).sum(axis=(1, 4))                       # (T, 3, F)
    if drop_last_corner:
        per_corner = per_corner.copy()
        val = valence(s)
        vert = s.tri.T.reshape(-1)                                   # corner i = k F + f -> its vertex
        for v in np.nonzero(val % 2 == 1)[0]:
            per_corner.reshape(s.T, -1)[:, np.nonzero(vert == v)[0][-1]] = 0.0
    nrm = np.sqrt(s.c2v_one_T.dot(per_corner.reshape(-1)).reshape(s.T, s.V) + w_end ** 2)
    return w_fst, w_end, w_mid, nrm


def cone_masks(s):
    """Which branch the oracle's projection takes at every (t, v) of the state ``s`` holds, and which columns sit exactly on a boundary."""
    w_fst, w_end, w_mid, nrm = cone_preimage(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.clip(0.5 * (1.0 + w_fst / nrm), 0.0, 1.0)
    corner_max = s.c2v_one_T.dot(np.abs(w_mid).max(axis=(1, 4)).reshape(-1)).reshape(s.T, s.V)
    return dict(lam=lam, one=lam >= 1.0, zero=lam == 0.0, mid=(lam > 0.0) & (lam < 1.0), nan=np.isnan(lam),
                on_upper=(w_fst == nrm) & (nrm > 0.0), on_lower=(w_fst == -nrm) & (nrm > 0.0),
                zero_preimage=(w_fst == 0.0) & (w_end == 0.0) & (corner_max == 0.0))


def project(s, mutation=None):
    """The oracle's projection on ``s``; ``mutation`` names a deliberate defect of a kernel:
    ``one_branch``   z_fst = lam * nrm also where lam was clipped to 1;
    ``drops_nan``    fmin / fmax semantics: the 0 / 0 column comes out as lam = 0;
    ``odd_tail``     the last interval of an odd T is not written (z_fst and z_end keep what they held);
    ``last_corner``  the last corner of an odd-valence vertex is left out of the norm."""
    old = (s.z_fst.copy(), s.z_end.copy())
    w_fst, w_end, w_mid, nrm = cone_preimage(s, drop_last_corner=mutation == "last_corner")
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.clip(0.5 * (1.0 + w_fst / nrm), 0.0, 1.0)
    if mutation == "drops_nan":
        lam = np.where(np.isnan(lam), 0.0, lam)
    lam_corner = s.v2c_T.dot(lam.reshape(-1)).reshape(s.T, 3, s.F) / s.D[None]
    with np.errstate(invalid="ignore"):
        s.z_fst[:] = lam * nrm if mutation == "one_branch" else np.where(lam >= 1.0, w_fst, lam * nrm)
        s.z_mid[:] = lam_corner[:, None, :, :, None] * w_mid
        s.z_end[:] = lam * w_end
    if mutation == "odd_tail" and s.T % 2 == 1:
        s.z_fst[-1], s.z_end[-1] = old[0][-1], old[1][-1]


def oracle_step(s, before, mutation=None, palm=False):
    """One iteration of the oracle from ``before`` (with the defect ``mutation`` of ``project``); returns the state after it."""
    load(s, before)
    if palm:
        palm_step0(s)
    s.step_laplacian()
    if mutation is None:
        s.step_soc_projection()
    else:
        project(s, mutation)
    s.step_q_lambda()
    s.step_multipliers()
    return snapshot(s)


def palm_step0(s):
    """is_palm's step 0 as the device runs it: the closed form with the gradients of the phi in memory."""
    s.dt_phi = O.grad_time(s.h, s.phi)
    s.dx_phi = O.grad_space(s.G, s.F, s.phi)
    s.step_q_lambda(refresh_gradients=False)


def apply_penalty(s, before, factor, skip=()):
    """``before`` after the oracle's adjust_penalty(factor) (which also moves s.r and the boundary term); ``skip``: dual arrays the
    division forgets (a deliberate mutation)."""
    load(s, before)
    s.adjust_penalty(factor)
    out = snapshot(s)
    for k in skip:
        out[k] = np.array(before[k], copy=True)
    return out


# ---- the state ------------------------------------------------------------------------------------------------------------
def _undivided(x, div):
    """A double y with y / div == x exactly (the pending division brings the planted value back), or None."""
    y = x * div
    for cand in (y, np.nextafter(y, np.inf), np.nextafter(y, -np.inf), np.nextafter(np.nextafter(y, np.inf), np.inf),
                 np.nextafter(np.nextafter(y, -np.inf), -np.inf)):
        if cand / div == x:
            return float(cand)
    return None


def default_cells(T):
    """Where ``edge_state`` plants its special columns unless told otherwise: name -> interval (nan*: a zero pre-image, up* / lo*: exactly
    on the upper / lower boundary of the cone)."""
    return {"nan0": 0, "nan1": T - 1, "up0": 0, "up1": T - 1, "lo0": T // 2, "lo1": T - 1}


def edge_state(s, seed, zero_preimage=True, div=1.0, cells=None):
    """Fill the twelve arrays of ``s`` by the recipe of random_state (test_hip_phases.py), then overwrite single (v, t) columns so that the
    oracle's own projection
      * takes each branch (lam clipped to 1, clipped to 0, in between) on about a third of all columns, chosen entry by entry;
      * sits exactly on the boundary w_fst == nrm (lam = 1.0) on two columns and on w_fst == -nrm (lam = 0.0) on two more: all corner
        entries 0, A = 0 and beta_fst == beta_end, so that w_fst == w_end and nrm = sqrt(w_end^2) = |w_end| exactly;
      * ``zero_preimage``: has a zero pre-image (lam = 0 / 0 = NaN in the reference) on one column at t = 0 (even) and one at the last
        interval (the lane without a second interval when T is odd).
    ``div`` != 1: the five dual arrays are left as they stand BEFORE a penalty division by ``div`` that is still to come
    (adjust_penalty(div) on ``s`` and on the device): the properties hold for the divided state.
    ``cells``: name -> interval of the special columns (``default_cells`` when None; any number of names that start with nan, up or lo,
    at most V - 1 of them): a time slab's tests put them next to the slab boundaries.
    Returns the masks of ``cone_masks`` for the state the iteration sees, plus ``planted``: the (t, v) of the special columns."""
    rng = np.random.default_rng(seed)
    for k in STATE:
        setattr(s, k, rng.standard_normal(getattr(s, k).shape))
    s.beta_fst[:, ::3] -= 6.0
    s.beta_fst[:, 1::3] += 6.0
    T, V = s.T, s.V
    val = valence(s)
    v_odd = int(np.argmax(np.where(val % 2 == 1, val, -1)))          # the vertex of the largest odd valence stays an ordinary column
    where = default_cells(T) if cells is None else dict(cells)
    assert len(where) <= V - 1 and all(k[:2] in ("na", "up", "lo") and 0 <= t < T for k, t in where.items()), where
    vs = [int(v) for v in rng.permutation(V) if v != v_odd][:len(where)]
    if cells is None:      # (the order the vertices were always dealt in)
        where = {k: where[k] for k in ("nan0", "nan1", "up0", "up1", "lo0", "lo1")}
    cells = {k: (int(t), v) for (k, t), v in zip(where.items(), vs)}
    if not zero_preimage:
        cells = {k: tv for k, tv in cells.items() if not k.startswith("nan")}
    d_pre = _undivided(s.d, div)
    assert d_pre is not None, "no double divides back to const_d"
    vert = s.tri.T                                                  # (3, F): vertex of corner (k, f)
    for name, (t, v) in cells.items():
        faces = np.nonzero((s.tri == v).any(axis=1))[0]
        s.B[t:t + 2, faces] = 0.0                                   # nodes t and t + 1 of its triangles
        own = vert == v                                             # its corners
        s.beta_mid[t][:, own] = 0.0
        s.A[t, v] = 0.0
        if name.startswith("nan"):
            s.beta_fst[t, v] = s.beta_end[t, v] = d_pre             # w_fst = w_end = d - d = 0
        elif name.startswith("up"):
            s.beta_fst[t, v] = s.beta_end[t, v] = (s.d - 3.0) * div  # w_fst = w_end > 0
        else:
            s.beta_fst[t, v] = s.beta_end[t, v] = (s.d + 3.0) * div  # w_fst = w_end < 0
    # every other column: beta_fst alone places w_fst against the norm (which does not depend on beta_fst)
    keep = snapshot(s)
    for k in DUAL:
        if k != "beta_fst":
            setattr(s, k, getattr(s, k) / div)
    nrm = cone_preimage(s)[3]
    load(s, keep)
    special = set((int(t), int(v)) for t, v in cells.values())
    rest = [(t, v) for t in range(T) for v in range(V) if (t, v) not in special]
    rest = [rest[j] for j in rng.permutation(len(rest))]
    rest.sort(key=lambda tv: tv != (T - 1, v_odd))                   # first, so in between: the whole corner list of an odd valence matters there
    for i, (t, v) in enumerate(rest):
        u = rng.uniform()
        ratio = (0.8 * (2.0 * u - 1.0), 1.5 + u, -1.5 - u)[i % 3]
        s.beta_fst[t, v] = (s.d - s.sz * s.A[t, v] - ratio * nrm[t, v]) * div
    keep = snapshot(s)
    for k in DUAL:
        setattr(s, k, getattr(s, k) / div)
    masks = cone_masks(s)
    load(s, keep)
    masks["planted"] = {k: (int(t), int(v)) for k, (t, v) in cells.items()}
    return masks


def assert_edge_properties(masks, zero_preimage=True, cells=None, boundary=()):
    """Conditions on the INPUT (the oracle's own lam), not on the device.  ``cells``: where the special columns were asked for, when not
    at ``default_cells``; ``boundary``: intervals next to a slab boundary, where every branch must occur on at least one column."""
    n = masks["lam"].size
    T = masks["lam"].shape[0]
    cells = masks.get("cells") if cells is None else cells          # (what the side under test asked _upload for)
    boundary = boundary or masks.get("boundary", ())
    for branch in ("one", "zero", "mid"):
        assert masks[branch].sum() >= 0.1 * n, (branch, int(masks[branch].sum()), n)
    assert (masks["on_upper"] & (masks["lam"] == 1.0)).sum() >= 2 and (masks["on_lower"] & (masks["lam"] == 0.0)).sum() >= 2
    both = masks["nan"] & masks["zero_preimage"]
    if zero_preimage:
        if cells is None:
            assert both[0].any() and both[T - 1].any()
        assert both.sum() >= 2
        assert np.array_equal(masks["nan"], masks["zero_preimage"])
    else:
        assert not masks["nan"].any()
    # the planted columns are where they were asked for
    want = default_cells(T) if cells is None else cells
    want = {k: t for k, t in want.items() if zero_preimage or not k.startswith("nan")}
    assert set(masks["planted"]) == set(want), (sorted(masks["planted"]), sorted(want))
    for k, (t, v) in masks["planted"].items():
        assert t == want[k], (k, t, want[k])
        if k.startswith("nan"):
            assert both[t, v], k
        elif k.startswith("up"):
            assert masks["on_upper"][t, v] and masks["lam"][t, v] == 1.0, k
        else:
            assert masks["on_lower"][t, v] and masks["lam"][t, v] == 0.0, k
    for t in boundary:
        for branch in ("one", "zero", "mid"):
            assert masks[branch][t].any(), (branch, t)


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def compare_entries(name, got, want, tol=FP_TOL):
    """Entry by entry: NaN where and only where the oracle has NaN; finite entries within tol * max(|want|, rms of the finite entries)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (name, "NaN positions differ", int(np.isnan(got).sum()), int(nan.sum()))
    fin = ~nan
    if not fin.any():
        return 0.0
    rms = float(np.sqrt(np.mean(want[fin] ** 2)))
    err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), max(rms, 1e-300))
    worst = float(err.max())
    assert worst <= tol, (name, worst, tuple(int(i) for i in np.argwhere(fin)[int(err.argmax())]))
    return worst


def check_one_step(s, before, after, phi_tol=PHI_TOL, palm=False, skip=()):
    """``after`` is ``before`` one ALM iteration later.  The oracle ``s`` (parameters already those of the iteration) forms phi from
    ``before``; after["phi"] must agree within ``phi_tol`` (gauge removed when eps == 0).  The oracle then CONTINUES FROM after["phi"]
    -- the solve's conditioning stays out of what follows -- and the other eleven arrays are compared entry by entry (``compare_entries``).
    ``palm``: is_palm's step 0 first.  ``skip``: arrays ``after`` does not hold (z_mid after a DOTS_STEP_SKIP_Z_MID step).
    Returns the worst figure per array; leaves the oracle holding ITS state after the iteration."""
    load(s, before)
    if not palm:
        s.z_mid = np.zeros_like(s.z_mid)      # (possibly stale on the device: the projection overwrites it before anything reads it)
    for k in STATE:
        assert np.isfinite(getattr(s, k)).all(), (k, "not finite before the step")
    if palm:
        palm_step0(s)
    s.step_laplacian()
    got, want = np.asarray(after["phi"]), s.phi
    assert got.shape == want.shape and np.isfinite(got).all(), "phi"
    if s.eps == 0.0:
        w = np.broadcast_to(s.mass_v[None, :], got.shape)
        got_c, want_c = got - np.sum(got * w) / np.sum(w), want - np.sum(want * w) / np.sum(w)
    else:
        got_c, want_c = got, want
    figures = {"phi": float(np.max(np.abs(got_c - want_c)) / max(np.max(np.abs(want_c)), 1e-300))}
    assert figures["phi"] < phi_tol, ("phi", figures["phi"])
    s.phi[:] = got
    s.step_soc_projection()
    s.step_q_lambda()
    s.step_multipliers()
    for k in STATE[1:]:
        if k not in skip:
            figures[k] = compare_entries(k, after[k], getattr(s, k))
    return figures


def compare_kkt(s, after, got, conditions=(0, 1, 2, 3, 6)):
    """dev.kkt(conditions) against the oracle's closures evaluated on ``after``."""
    load(s, after)
    s.dt_phi = O.grad_time(s.h, s.phi)
    s.dx_phi = O.grad_space(s.G, s.F, s.phi)
    s.dec_B = O.decouple(s.B, s.sz)
    fns = s.kkt_functions()
    for i in conditions:
        want = fns[i]()
        for j in range(2 if i < 4 else 1):
            assert np.isfinite(want[j]) and abs(got[i][j] - want[j]) <= KKT_TOL * abs(want[j]), (i, j, got[i][j], want[j])


# ---- the CPU stand-in for the calls the scenarios make -------------------------------------------------------------------------
def refused(status, what):
    """The error a refused call raises, as ``_lib.check`` raises it."""
    from dots_socp_amd import _lib

    err = _lib.HipLibraryError(f"{what} failed with status {status}")
    err.status = status
    return err


def trace_host(mu, E, triangles, n_vertices, tables, start_triangle, start_weights, neighbours, floor, span, action=False, mass=None,
               max_crossings=16, slide=False):
    """What ``DeviceProblem.flow_trace`` returns without a trajectory, from the host specifications (flow.flow_map_host and, with a
    ``mass``, flow.push_forward_host on the last layer); ``tables``: ``(areas, hat)`` in the caller's triangle numbering."""
    from dots_socp_amd import flow

    areas, hat = tables
    out = flow.flow_map_host(mu, E, triangles, hat, neighbours, start_triangle, start_weights, floor, max_crossings=max_crossings, trajectory=True,
                             span=tuple(int(n) for n in span), action=action, slide=slide, areas=areas if slide else None)
    if mass is not None:
        k = flow.push_scales(mass, None, start_weights)
        pushed = flow.push_forward_host(out, triangles, n_vertices, mass, None, k, "end")
        out.update(mass_at=pushed["mass"], attr_at=None, dropped=pushed["dropped"], exponents=k)
    return {k: v for k, v in out.items() if k not in ("triangles_at", "weights_at")}


class OracleDevice:
    """``DeviceProblem``'s calls used below and by tests/sequence_checks.py, played by a second oracle (tests/fake_device.py plays time
    slabs only: no upload, no dots_step).  It knows nothing of kernels: counter 12 is not played, and every hint of ``step_flags`` is
    taken and ignored.  What the header documents about z_mid is played: after a step with ``skip_z_mid`` the calls that read it are
    refused with DOTS_ERR_STATE until a step without the flag, an upload of it or the projection phase."""

    NORMS = {"phi": "nsq_center", "A": "nsq_time", "lambda_c": "nsq_time", "mu": "nsq_time", "z_fst": "nsq_time", "z_end": "nsq_time",
             "beta_fst": "nsq_time", "beta_end": "nsq_time", "B": "nsq_space", "E": "nsq_space", "z_mid": "nsq_space_dec", "beta_mid": "nsq_space_dec"}
    PARAMS = {"r": "r", "scale_z": "sz", "const_d": "d", "norm_d": "norm_d"}      # dots_params -> the oracle's attribute

    def __init__(self, T, geom, congestion, strict=True):
        self.s = make_oracle(T, geom, congestion)
        self.strict = strict
        self.palm = False
        self.skip = False
        self.stale = False      # z_mid unspecified (the last step ran with skip_z_mid)
        self.geom = geom
        self.norm_d0 = self.s.norm_d / 1.3      # (as a new context has it: make_oracle scaled it)

    # ---- state transfer
    def upload(self, name, a):
        setattr(self.s, name, np.array(a, dtype=np.float64, copy=True))
        if name == "z_mid":
            self.stale = False

    def download(self, name):
        if name == "z_mid" and self.stale:
            raise refused(-5, "download z_mid")
        return getattr(self.s, name).copy()

    def download_all(self):
        return {k: self.download(k) for k in STATE}

    # ---- parameters and scaling tools
    def set_params(self, **kw):
        """The scenarios (``strict``) only ever bring the ``r`` that adjust_penalty moved already.  Otherwise the scalars are the
        caller's, as on the device: ``r`` is the penalty the state is read with, and the boundary term follows it."""
        s = self.s
        if self.strict:
            assert set(kw) == {"r"} and abs(kw["r"] - self.s.r) <= 1e-15 * self.s.r      # (adjust_penalty moved it already)
            return
        for k, v in kw.items():
            if k == "r":
                s.bnd *= s.r / v
                s.r = float(v)
            elif k in self.PARAMS:
                setattr(s, self.PARAMS[k], float(v))
            else:
                assert k in ("congestion", "tau") or (k == "eps" and v == s.eps), k      # (eps is built into the oracle's solve)
                setattr(s, k, float(v))

    def adjust_penalty(self, f):
        self.s.adjust_penalty(f)

    def scale_z(self, z_mul, beta_mul, scale_z_new):
        """The arrays only, as the header states it (the caller brings scale_z, const_d and norm_d with set_params)."""
        s = self.s
        for k in ("z_fst", "z_mid", "z_end"):
            setattr(s, k, getattr(s, k) * z_mul)
        for k in ("beta_fst", "beta_mid", "beta_end"):
            setattr(s, k, getattr(s, k) * beta_mul)
        s.mu = scale_z_new * (s.beta_fst - s.beta_end)
        s.E = -O.decouple_adjoint(s.beta_mid, scale_z_new)

    def scale_arrays(self, names, factor):
        for k in names:
            setattr(self.s, k, getattr(self.s, k) * factor)

    # ---- the iteration
    def step_flags(self, palm=False, skip_z_mid=False, rhs_ahead=False, **_hints):
        if palm and (skip_z_mid or rhs_ahead):
            raise refused(-1, "dots_step_flags")
        self.palm, self.skip = palm, skip_z_mid

    def step(self, n=1, wait=True):
        for _ in range(n):
            if self.palm:
                if self.stale:
                    raise refused(-5, "dots_step")
                palm_step0(self.s)
            self.s.iterate()
            self.stale = self.skip

    def run_phase(self, phase):
        s = self.s
        if phase == "laplacian":
            s.step_laplacian()
        elif phase == "soc_projection":
            s.step_soc_projection()
            self.stale = False
        elif phase == "q_lambda_mult":
            s.step_q_lambda()
            s.step_multipliers()
        else:
            assert phase == "q_lambda", phase
            if self.stale:
                raise refused(-5, "phase q_lambda")
            palm_step0(s)

    # ---- what is read
    def kkt(self, conditions):
        s = self.s
        conditions = list(conditions)
        if 1 in conditions and self.stale:
            raise refused(-5, "dots_kkt")
        s.dt_phi = O.grad_time(s.h, s.phi)      # (of the phi in memory, as the device forms them)
        s.dx_phi = O.grad_space(s.G, s.F, s.phi)
        s.dec_B = O.decouple(s.B, s.sz)
        fns = s.kkt_functions()
        return {i: list(fns[i]()) for i in conditions}

    def objective(self):
        return self.s.objective()

    def norm_square(self, name, part=0):
        s = self.s
        if name == "z_mid" and self.stale:
            raise refused(-5, "dots_norm_square")
        if name == "phi" and part == 1:
            return s.nsq_time(O.grad_time(s.h, s.phi))
        if name == "phi" and part == 2:
            return s.nsq_space(O.grad_space(s.G, s.F, s.phi))
        return getattr(s, self.NORMS[name])(getattr(s, name))

    def apply_operator(self, op, x, scale=1.0):
        s = self.s
        x = np.asarray(x, dtype=np.float64)
        return {"grad_time": lambda: O.grad_time(s.h, x), "div_time": lambda: O.div_time(s.h, x), "grad_space": lambda: O.grad_space(s.G, s.F, x),
                "div_space": lambda: O.div_space(s.Dv, x), "decouple": lambda: O.decouple(x, scale), "decouple_adjoint": lambda: O.decouple_adjoint(x, scale),
                "time_avg_adjoint": lambda: O.time_average_adjoint(x)}[op]()

    def readout(self, factor=1.0, w_vertex=None, w_triangle=None, centred=False, mu0=None, mu1=None):
        from dots_socp_amd import readout

        mu, E = readout.read_out_host({"mu": self.s.mu, "E": self.s.E}, factor, w_vertex, w_triangle, centred, mu0, mu1)
        return (mu, E) + tuple(readout.layer_sums_host(mu))

    def sensitivity(self, factor_phi=1.0, factor_mu=1.0, mass_vertex=None):
        from dots_socp_amd import sensitivity

        s = self.s
        phi0, phiT = sensitivity.potentials_host(s.phi, factor_phi)
        mass = s.mass_v if mass_vertex is None else mass_vertex
        return {"phi0": phi0, "phiT": phiT, "stress": sensitivity.stress_numpy(s.mu, s.phi, s.tri, mass, factor_mu, factor_phi)}

    def flow_tables(self):
        """``(areas, hat)`` of the host specification of the tracer: this stand-in's own (a device holds its plan's)."""
        from dots_socp_amd.geometry import hat_gradients

        return hat_gradients(self.geom["vertices"], self.geom["triangles"])

    def flow_trace(self, start_triangle, start_weights, neighbours, floor, span, action=False, mass=None, max_crossings=16, slide=False):
        s = self.s
        return trace_host(s.mu, s.E, s.tri, s.V, self.flow_tables(), start_triangle, start_weights, neighbours, floor, span, action=action,
                          mass=mass, max_crossings=max_crossings, slide=slide)

    def flow_map(self, start_triangle, start_weights, neighbours, floor, max_crossings=16, slide=False):
        return self.flow_trace(start_triangle, start_weights, neighbours, floor, (0, self.s.T), max_crossings=max_crossings, slide=slide)

    def flow_push(self, start_triangle, start_weights, neighbours, floor, mass, max_crossings=16):
        return self.flow_trace(start_triangle, start_weights, neighbours, floor, (0, self.s.T), mass=mass, max_crossings=max_crossings)

    # ---- solve session
    def restart(self, mu0, mu1, mode="cold", factors=None):
        """dots_restart as the header states it: new end masses, the parameters of a new context (tau and eps kept), the state zeroed
        (cold) or every array times the factor of its group (warm; refused while z_mid is unspecified)."""
        s = self.s
        if mode == "warm" and self.stale:
            raise refused(-5, "dots_restart")
        groups = (("phi", "A", "B", "lambda_c"), ("z_fst", "z_mid", "z_end"), ("mu", "E"), ("beta_fst", "beta_mid", "beta_end"))
        for group, f in zip(groups, factors if mode == "warm" else (0.0,) * 4):
            for k in group:
                setattr(s, k, getattr(s, k) * f if mode == "warm" else np.zeros_like(getattr(s, k)))
        s.r, s.sz, s.d, s.congestion, s.norm_d = 1.0, 1.0, 1.0, 0.0, self.norm_d0
        s.bnd = np.zeros_like(s.bnd)
        s.bnd[0] = -np.asarray(mu0, dtype=np.float64) / s.h
        s.bnd[-1] = np.asarray(mu1, dtype=np.float64) / s.h
        s.norm_boundary = s.h * float(np.sqrt(s.nsq_center(s.bnd / s.w_v)))
        self.palm = self.skip = self.stale = False

    def penalty_ahead(self, *policy):
        pass      # (a hint)

    def close(self):
        pass


# ---- the scenarios --------------------------------------------------------------------------------------------------------------
# Every scenario: (dev, s, T, seed, expect) -> None.  ``dev`` holds the parameters of ``s``; ``expect(dev, **bits)`` asserts on
# dots_debug_counter 12 that the step just enqueued took the named launches (a no-op on the CPU).
def _upload(dev, s, seed, **kw):
    """``dev.cells`` / ``dev.boundary`` (a time slab's adapter has them): where the special columns go, and the intervals next to a slab
    boundary that ``assert_edge_properties`` then looks at."""
    masks = edge_state(s, seed, cells=getattr(dev, "cells", None), **kw)
    masks["cells"], masks["boundary"] = getattr(dev, "cells", None), tuple(getattr(dev, "boundary", ()))
    before = snapshot(s)
    for k in STATE:
        dev.upload(k, before[k])
    return before, masks


def _after(dev, skip=()):
    return {k: dev.download(k) for k in STATE if k not in skip}


def _two_branches(s):
    """A state one iteration after a planted one cannot be planted again (an upload drops what the step carried).  The multiplier update has
    pulled every column off the lam = 1 branch by then; what the second step of a scenario must still see is lam = 0 and 0 < lam < 1."""
    m = cone_masks(s)
    return bool(m["zero"].sum() >= 0.1 * m["lam"].size and m["mid"].sum() >= 0.1 * m["lam"].size)


def scenario_plain(dev, s, T, seed, expect):
    """a. No flags: the right-hand side with the projection riding along, k_q_lambda_mult_triangle2<1>."""
    before, masks = _upload(dev, s, seed)
    assert_edge_properties(masks)
    dev.step_flags()
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_triangle2", z=1)
    check_one_step(s, before, _after(dev))


def scenario_skip_z_mid(dev, s, T, seed, expect):
    """b. DOTS_STEP_SKIP_Z_MID (Z = 2: z_mid rebuilt in registers, never stored), then a step that stores it again."""
    before, masks = _upload(dev, s, seed, zero_preimage=False)
    assert_edge_properties(masks, zero_preimage=False)
    dev.step_flags(skip_z_mid=True)
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_triangle2", z=2)
    after = _after(dev, skip=("z_mid",))
    check_one_step(s, before, after, skip=("z_mid",))
    before = dict(after, z_mid=np.full_like(before["z_mid"], np.nan))      # stale on the device: nothing may read it
    load(s, dict(before, z_mid=s.z_mid))
    assert _two_branches(s)
    dev.step_flags()
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_triangle2", z=1)
    check_one_step(s, before, _after(dev))


def scenario_carry(dev, s, T, seed, expect):
    """c. DOTS_STEP_CARRY, two steps: the second streams cn_sq and cn_g (the downloads in between keep them)."""
    before, masks = _upload(dev, s, seed, zero_preimage=False)
    assert_edge_properties(masks, zero_preimage=False)
    dev.step_flags(carry=True)
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_carry", z=2, defer=True)
    after = _after(dev)
    check_one_step(s, before, after)
    load(s, after)
    assert _two_branches(s)
    dev.step(1, wait=False)
    expect(dev, carried=True, rider=True, ql="ql_carry", z=2, defer=True)
    check_one_step(s, after, _after(dev))


def scenario_carry_kkt(dev, s, T, seed, expect):
    """d. DOTS_STEP_CARRY + DOTS_STEP_KKT_SUMS: K = 1, and the residuals read from the fused sums."""
    before, masks = _upload(dev, s, seed, zero_preimage=False)
    assert_edge_properties(masks, zero_preimage=False)
    dev.step_flags(carry=True, kkt_sums=True)
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_carry", z=2, kkt=True, defer=True)
    got = dev.kkt([0, 1, 2, 3, 6])          # (before any download: from the sums steps 2+3 left)
    after = _after(dev)
    check_one_step(s, before, after)
    compare_kkt(s, after, got)


def _pending(dev, s, before):
    dev.adjust_penalty(FACTOR)
    dev.set_params(r=s.r * FACTOR)
    return apply_penalty(s, before, FACTOR)      # (moves s.r and the boundary term too)


def scenario_pending_division(dev, s, T, seed, expect):
    """e. A penalty division left pending: both launches divide as they read (DIV), nothing carried, z_mid deferred -- and rebuilt for the
    download from the OLD, still undivided beta_mid."""
    before, masks = _upload(dev, s, seed, div=FACTOR)
    assert_edge_properties(masks)
    before = _pending(dev, s, before)
    dev.step_flags(carry=True)
    dev.step(1, wait=False)
    expect(dev, div=True, rider=True, ql="ql_carry", z=2, ql_div=True, defer=True)
    check_one_step(s, before, _after(dev))


def scenario_pending_division_kkt(dev, s, T, seed, expect):
    """e'. The same with DOTS_STEP_KKT_SUMS alone: the carry kernel without the carry (emit = 2)."""
    before, masks = _upload(dev, s, seed, div=FACTOR)
    assert_edge_properties(masks)
    before = _pending(dev, s, before)
    dev.step_flags(kkt_sums=True)
    dev.step(1, wait=False)
    expect(dev, div=True, rider=True, ql="ql_carry", z=2, kkt=True, ql_div=True, defer=True)
    check_one_step(s, before, _after(dev))


def scenario_pending_after_carry(dev, s, T, seed, expect):
    """f. A pending division after a carried step: the carried sums are dropped (CARRIED = 0, DIV = 1)."""
    before, masks = _upload(dev, s, seed, zero_preimage=False)
    assert_edge_properties(masks, zero_preimage=False)
    dev.step_flags(carry=True)
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_carry", z=2, defer=True)
    after = _after(dev)
    check_one_step(s, before, after)
    before = _pending(dev, s, after)
    assert _two_branches(s)
    dev.step(1, wait=False)
    expect(dev, div=True, rider=True, ql="ql_carry", z=2, ql_div=True, defer=True)
    check_one_step(s, before, _after(dev))


def scenario_timed(dev, s, T, seed, expect):
    """g. The synchronous, timed dots_step: right-hand side, solve, k_soc_projection, steps 2+3 as four phases."""
    before, masks = _upload(dev, s, seed)
    assert_edge_properties(masks)
    dev.step_flags()
    dev.step(1)
    expect(dev, rider=False, ql="ql_triangle2", z=1)
    check_one_step(s, before, _after(dev))


def scenario_timed_carry(dev, s, T, seed, expect):
    """g'. ... with DOTS_STEP_CARRY: the second step's stand-alone projection and right-hand side stream the carried sums."""
    before, masks = _upload(dev, s, seed, zero_preimage=False)
    assert_edge_properties(masks, zero_preimage=False)
    dev.step_flags(carry=True)
    dev.step(1)
    expect(dev, rider=False, ql="ql_carry", z=2, defer=True)
    after = _after(dev)
    check_one_step(s, before, after)
    load(s, after)
    assert _two_branches(s)
    dev.step(1)
    expect(dev, carried=True, rider=False, ql="ql_carry", z=2, defer=True)
    check_one_step(s, after, _after(dev))


def scenario_palm(dev, s, T, seed, expect):
    """g''. is_palm: step 0 (the closed form on the stored z_mid) opens the iteration."""
    before, masks = _upload(dev, s, seed)
    assert_edge_properties(masks)
    dev.step_flags(palm=True)
    dev.step(1, wait=False)
    expect(dev, rider=True, ql="ql_triangle2", z=1)
    check_one_step(s, before, _after(dev), palm=True)


SCENARIOS_ALL_T = {"plain": scenario_plain, "carry": scenario_carry, "pending_division": scenario_pending_division}
SCENARIOS_FEW_T = {"skip_z_mid": scenario_skip_z_mid, "carry_kkt": scenario_carry_kkt, "pending_division_kkt": scenario_pending_division_kkt,
                   "pending_after_carry": scenario_pending_after_carry, "timed": scenario_timed, "timed_carry": scenario_timed_carry,
                   "palm": scenario_palm}


def cases():
    """(scenario, mesh, T, congestion): a, c and e on every mesh and T, the rest on one small-pitch and one matrix-core T per mesh."""
    out = []
    for table, ts in ((SCENARIOS_ALL_T, T_ALL), (SCENARIOS_FEW_T, T_FEW)):
        for name in table:
            for mesh in MESHES:
                for T in ts:
                    for congestion in (0.0, 0.05):
                        out.append((name, mesh, T, congestion))
    return out


def scenario(name):
    return SCENARIOS_ALL_T.get(name) or SCENARIOS_FEW_T[name]
