"""The KKT, objective and norm sums slot by slot (plain numpy, TEST INFRASTRUCTURE shared by test_kkt_checks_cpu.py and
test_hip_kkt_slots.py).

The seven residuals are ratios ``res / (c + nsum)`` of square roots of 22 weighted sums of squares; an error in one sum can hide behind
the constant or behind a norm sum of the denominator.  Here every sum is compared on its own with an extended-precision evaluation:

``SLOTS``, ``NEEDS``  the 22 names in the device's order (csrc/dots_dev.h) and the conditions that form each;
``reference``         every KKT slot, the three objective sums and ``norm_square`` of the twelve arrays (plus parts 1 and 2 of phi) in
                      np.longdouble, from the formulas of the reference solver (solver_socp.py:417-559, :875-878) with the oracle's geometry
                      tables, each with a running error bound for an fp64 evaluation; a time slab's share with ``slab`` / ``halos``;
``plain``             the same sums in fp64 numpy in the straightforward order, with knobs for deliberate defects (``MUTATIONS``);
``tolerances``        MARGIN * max(|plain - reference|, bound) per slot: nothing in it comes from the side under test;
``combine``           the seven residuals from the slots (the reference's closures), the link to ``OracleSolver.kkt_functions``;
``white``, ``converged``, ``probe``   the states.

THE BOUND.  An entry e of a sum is an expression of n roundings over terms t_i: an fp64 evaluation is off by at most u n sum|t_i|,
u = 2^-53 (to first order; n counted from the mathematical expression, a corner walk of valence k counts its k additions; the count
includes the roundings of the geometry tables the expression reads: TAB_AREA for a triangle area, TAB_AREA + k + 1 for a vertex mass of
valence k, TAB_HAT for a hat gradient (of the size of the gradient vector) -- the device holds tables formed by the library's host assembly in its own numbering, which
agree with the oracle's to that many roundings, as test_kkt_checks_cpu.py asserts).  The entry contributes e^2 w: the error of the
entry goes through the square ((2|e| de + de^2) w) and the square and the weight round once each (plus the weight's table roundings);
a sum of N entries adds N u times the sum.  The norms divide once more.
"""
import os
import re

import numpy as np

import step_checks as sc

O = sc.O
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "kkt_checks needs an extended-precision long double (x87: 64-bit mantissa)"

MARGIN = 16.0      # the margin of mode_checks
U = 2.0 ** -53
TAB_AREA, TAB_HAT = 8, 16      # roundings of 0.5 |e1 x e2| and of alt / |alt|^2 from the vertex positions (see the module docstring)
STATE = sc.STATE

SLOTS = ("V_DPHI2", "V_A2", "V_LAM2", "V_RESMU2", "V_RFST2", "V_REND2", "V_MU2", "V_AUX1_2", "V_MUAUX1_2", "V_COMP_AUX2", "V_COMP_RES2",
         "V_CONG_RES2", "V_DUALAUX2", "F_DX2", "F_B2", "F_RESE2", "F_E2", "F_AUX2_2", "F_EAUX2_2", "F_AUX5_2", "F_AUX5M_2", "F_RMID2")
N_SUMS = len(SLOTS)
IX = {k: i for i, k in enumerate(SLOTS)}
# the conditions (0 Prim(phi, q), 1 Prim(q, z), 2 Dual(alpha), 3 Dual(beta), 4 Comp(rho, f(q)), 5 Comp(m, rho o B), 6 Comp(rho, cong.))
# whose closure reads the slot (solver_socp.py:433-559)
NEEDS = {"V_DPHI2": (0,), "V_A2": (0,), "V_LAM2": (0, 6), "V_RESMU2": (0,), "V_RFST2": (1,), "V_REND2": (1,), "V_MU2": (3, 4, 6),
         "V_AUX1_2": (3,), "V_MUAUX1_2": (3,), "V_COMP_AUX2": (4,), "V_COMP_RES2": (4,), "V_CONG_RES2": (6,), "V_DUALAUX2": (2,),
         "F_DX2": (0,), "F_B2": (0,), "F_RESE2": (0,), "F_E2": (3, 5), "F_AUX2_2": (3,), "F_EAUX2_2": (3,), "F_AUX5_2": (5,),
         "F_AUX5M_2": (5,), "F_RMID2": (1,)}
OBJECTIVE = ("phi0_mu0", "phiT_mu1", "lambda_c2")      # dots_objective_sums
# norm_square: (array, part) -> kind (0 node, 1 interval, 2 triangle, 3 corner)
NORMS = {("phi", 0): 0, ("phi", 1): 1, ("phi", 2): 2, ("A", 0): 1, ("lambda_c", 0): 1, ("mu", 0): 1, ("z_fst", 0): 1, ("z_end", 0): 1,
         ("beta_fst", 0): 1, ("beta_end", 0): 1, ("B", 0): 2, ("E", 0): 2, ("z_mid", 0): 3, ("beta_mid", 0): 3}

MUTATIONS = ("last_interval", "pair_reads_t1", "odd_corner", "mu1_sign", "mu0_interval", "ragged_tile", "neighbour_area", "rmid_last_half",
             "cong_prim_scale", "dphi_rounded", "objective_node", "norm_extra_column")
MUTATION_DOC = {
    "last_interval": "the last interval is left out of V_A2",
    "pair_reads_t1": "Comp(rho, f(q)): the second interval of an even/odd pair reads B of node t + 1 where it needs t + 2",
    "odd_corner": "Dual(alpha): the last corner of every odd-valence vertex is missing from the gather of E",
    "mu1_sign": "Dual(alpha): the mu1 term at the last node has the wrong sign",
    "mu0_interval": "Dual(alpha) at t = 0 subtracts mu[0]",
    "ragged_tile": "the V % VT vertices of a ragged last tile after the full ones (device numbering; the last vertex alone where one tile holds them all) are omitted from V_MU2",
    "neighbour_area": "component 2 of the last triangle (device numbering) is weighted in F_B2 with the area of the nearest triangle before it whose area differs by more than 1e-3",
    "rmid_last_half": "F_RMID2 is missing its (1, T - 1) half at the last node",
    "cong_prim_scale": "the congestion residual uses prim_scale for dual_scale",
    "dphi_rounded": "dphi is rounded to 1e-9 relative before the subtraction of V_RESMU2",
    "objective_node": "the objective reads phi of node T - 1",
    "norm_extra_column": "the corner kind of norm_square counts the column without an interval (played as the (1, T - 1) entries once more)",
}


def header_slots():
    """The enum V_DPHI2 ... N_SUMS as csrc/dots_dev.h spells it, without N_VSUMS and N_SUMS."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dots_socp_amd", "csrc", "dots_dev.h")
    with open(path) as fh:
        text = fh.read()
    body = re.search(r"enum\s*\{\s*(V_DPHI2.*?N_SUMS)\s*\}", text, re.S).group(1)
    names = [re.sub(r"\s*=.*", "", part.strip()) for part in body.split(",")]
    assert names[-1] == "N_SUMS" and "N_VSUMS" in names
    return [n for n in names if n not in ("N_VSUMS", "N_SUMS")], names.index("N_VSUMS")


def plane_geometry(n=20, seed=20):
    """meshes.plane(n) with positive end masses: n = 20 gives V = 504, F = 920, open (valences 1, 2, 3, 4 on the boundary, 6 inside)."""
    from dots_socp_amd import meshes

    v, t = meshes.plane(n)
    rng = np.random.default_rng(seed)
    mu0, mu1 = rng.uniform(0.5, 1.5, v.shape[0]), rng.uniform(0.5, 1.5, v.shape[0])
    return dict(vertices=v, triangles=t, mu0=mu0 / mu0.sum(), mu1=mu1 / mu1.sum())


# ---- parameters and numbering -----------------------------------------------------------------------------------------------------
def params_of(s, geom, boundary_scale=1.0):
    """What ``reference`` / ``plain`` read beside the state: the oracle's scalars as dots_params names them, and the end masses.
    boundary_scale: the oracle's boundary term is boundary_scale * (-mu0, +mu1) / (r h)."""
    return dict(r=s.r, scale_z=s.sz, const_d=s.d, congestion=s.congestion, prim_scale=s.prim_scale, dual_scale=s.dual_scale,
                boundary_scale=boundary_scale, mu0=np.asarray(geom["mu0"], dtype=np.float64), mu1=np.asarray(geom["mu1"], dtype=np.float64))


def device_params(s, p):
    """set_params' arguments for the state of ``s`` with the parameters ``p`` (``params_of``)."""
    return dict(r=p["r"], scale_z=p["scale_z"], const_d=p["const_d"], norm_d=s.norm_d, norm_boundary=s.norm_boundary, congestion=p["congestion"],
                eps=s.eps, tau=s.tau, prim_scale=p["prim_scale"], dual_scale=p["dual_scale"], boundary_scale=p["boundary_scale"])


def pitch_of(T):
    """csrc/dots_api.hip: the time pitch of a context on one GPU."""
    return max(8, 1 << int(T).bit_length())


class Numbering:
    """The device numbering of a plan: device vertex i = caller vertex perm_vert[i] (likewise triangles) and the tile heights."""

    def __init__(self, T, V, F, perm_vert=None, perm_tri=None):
        self.perm_vert = np.arange(V) if perm_vert is None else np.asarray(perm_vert, dtype=np.int64)
        self.perm_tri = np.arange(F) if perm_tri is None else np.asarray(perm_tri, dtype=np.int64)
        self.VT = self.FT = 1024 // pitch_of(T)
        self.n_vtiles, self.n_ftiles = -(-V // self.VT), -(-3 * F // self.FT)

    @classmethod
    def of_plan(cls, plan):
        return cls(plan.n_time, plan.n_vertices, plan.n_triangles, plan.perm_vert, plan.perm_tri)

    def last_tile_vertices(self):
        """Caller indices of the vertices of a ragged last vertex tile that follows full ones; the last device vertex alone where a
        single tile holds every vertex or no tile is ragged (a defect confined to a few entries either way)."""
        V = self.perm_vert.size
        return self.perm_vert[(V // self.VT) * self.VT:] if V % self.VT and V > self.VT else self.perm_vert[-1:]


# ---- the evaluation ---------------------------------------------------------------------------------------------------------------
def _corner_tables(s):
    """vertex of every corner j = 3 f + k, the valences, and the last corner (largest (k, f)) of every odd-valence vertex."""
    cv = s.tri.reshape(-1).astype(np.int64)
    val = np.bincount(cv, minlength=s.V)
    key = (np.arange(cv.size) % 3) * s.F + np.arange(cv.size) // 3
    last_odd = [int(np.nonzero(cv == v)[0][np.argmax(key[cv == v])]) for v in np.nonzero(val % 2 == 1)[0]]
    return cv, val, np.array(last_odd, dtype=np.int64)


def _gather(per_corner, cv, V):
    """out[t, v] = sum of per_corner[t, j] over the corners j of v."""
    out = np.zeros((per_corner.shape[0], V), dtype=per_corner.dtype)
    np.add.at(out, (slice(None), cv), per_corner)
    return out


def _round_rel(x, bits=30):
    m, e = np.frexp(x)
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


def _evaluate(s, state, params, X, bounds, mutation=None, slab=None, halos=None, numbering=None):
    assert mutation is None or mutation in MUTATIONS, mutation
    T, V, F = s.T, s.V, s.F
    a = {k: np.array(state[k], dtype=X) for k in STATE}
    n0, nl = (0, T + 1) if slab is None else (int(slab[0]), int(slab[1]))
    ni = max(0, min(nl, T - n0))
    if halos:      # what a slab received in place of its neighbours' entries: mu of interval n0 - 1, B and phi of node n0 + nl
        if halos.get("mu_lo") is not None and n0 > 0:
            a["mu"][n0 - 1] = np.asarray(halos["mu_lo"], dtype=X)
        if halos.get("B_hi") is not None and n0 + nl <= T:
            a["B"][n0 + nl] = np.asarray(halos["B_hi"], dtype=X).reshape(F, 3)
        if halos.get("phi_hi") is not None and n0 + nl <= T:
            a["phi"][n0 + nl] = np.asarray(halos["phi_hi"], dtype=X)
    phi, A, B, lc, zf, zm, ze, mu, E, bf, bm, be = (a[k] for k in STATE)
    r, sz, cd, cong, ps, ds, bs = (X(params[k]) for k in ("r", "scale_z", "const_d", "congestion", "prim_scale", "dual_scale", "boundary_scale"))
    h = X(1) / X(T)
    m, w, hat = s.mass_v.astype(X)[None, :], s.area_f.astype(X), s.hat.astype(X)
    wf = w[None, :, None]
    cv, val, last_odd = _corner_tables(s)
    tab_m = (TAB_AREA + val + 1)[None, :]      # roundings of a vertex mass
    I, N = slice(n0, n0 + ni), slice(n0, n0 + nl)
    sums, bnd_out = np.zeros(N_SUMS, dtype=X), np.zeros(N_SUMS, dtype=X)

    def put(slot, e, terms, n, weight, tab, rows, drop=None):
        """slot = sum over ``rows`` of e^2 weight; the entry is n roundings over terms of absolute sum ``terms``."""
        c = e * e * weight
        if drop is not None:
            c = drop(c)
        part = c[rows]
        sums[IX[slot]] = part.sum()
        if bounds:
            de = U * n * terms
            b = (2 * np.abs(e) * de + de * de) * weight + U * (2 + tab) * c
            bnd_out[IX[slot]] = b[rows].sum() + U * part.size * part.sum()

    # -- Prim(phi, q): dt_phi - A - lambda_c and dx_phi - B (solver_socp.py:433-450 with the residuals of :592-593)
    dphi, dphi_t = (phi[1:] - phi[:-1]) / h, (np.abs(phi[1:]) + np.abs(phi[:-1])) / h      # (h and 1 / h round: 4)
    put("V_DPHI2", dphi, dphi_t, 4, m, tab_m, I)
    put("V_A2", A, np.abs(A), 0, m, tab_m, I, drop=(lambda c: np.concatenate([c[:-1], 0 * c[-1:]])) if mutation == "last_interval" else None)
    put("V_LAM2", lc, np.abs(lc), 0, m, tab_m, I)
    put("V_RESMU2", (_round_rel(dphi) if mutation == "dphi_rounded" else dphi) - A - lc, dphi_t + np.abs(A) + np.abs(lc), 6, m, tab_m, I)
    gx = sum(hat[None, :, k, :] * phi[:, s.tri[:, k], None] for k in range(3))
    hat_s = np.broadcast_to(np.abs(hat).max(axis=2, keepdims=True), hat.shape)      # (a table entry is off by TAB_HAT u of the vector's size)
    gx_t = sum(np.abs(hat_s[None, :, k, :] * phi[:, s.tri[:, k], None]) for k in range(3))
    put("F_DX2", gx, gx_t, 3 + TAB_HAT, wf, TAB_AREA, N)
    wb = wf
    if mutation == "neighbour_area":
        wb = np.repeat(wf, 3, axis=2).copy()
        last, before = numbering.perm_tri[-1], numbering.perm_tri[-2::-1]
        wb[0, last, 2] = w[before[np.argmax(np.abs(w[before] - w[last]) > 1e-3 * w[last])]]      # (the nearest one before it of another size)
    put("F_B2", B, np.abs(B), 0, wb, TAB_AREA, N)
    put("F_RESE2", gx - B, gx_t + np.abs(B), 4 + TAB_HAT, wf, TAB_AREA, N)
    # -- Prim(q, z): z_fst + sz A - d, z_end - sz A - d, sz (z_mid - L B) (:452-464 with :598-600)
    put("V_RFST2", zf + sz * A - cd, np.abs(zf) + np.abs(sz * A) + abs(cd), 3, m, tab_m, I)
    put("V_REND2", ze - sz * A - cd, np.abs(ze) + np.abs(sz * A) + abs(cd), 3, m, tab_m, I)
    c3 = sz / np.sqrt(X(3))
    # (by the node an entry is compared with: [t][0] and [t - 1][1], as a slab owns them)
    rmid = np.zeros((T + 1, 2, 3, F, 3), dtype=X)
    rmid_t = np.zeros_like(rmid)
    rmid[:-1, 0], rmid[1:, 1] = sz * (zm[:, 0] - c3 * B[:-1, None]), sz * (zm[:, 1] - c3 * B[1:, None])
    rmid_t[:-1, 0], rmid_t[1:, 1] = np.abs(sz * zm[:, 0]) + np.abs(sz * c3 * B[:-1, None]), np.abs(sz * zm[:, 1]) + np.abs(sz * c3 * B[1:, None])
    if mutation == "rmid_last_half":
        rmid[T, 1] = 0
    put("F_RMID2", rmid, rmid_t, 5, w[None, None, None, :, None], TAB_AREA, N)
    # -- Dual(alpha): (r h) (bnd + div_time(mu m) + div_space(E w)) / m (:466-482)
    bnd = np.zeros((T + 1, V), dtype=X)
    bnd[0] = -bs * np.asarray(params["mu0"], dtype=X) / (r * h)
    bnd[T] = (-1 if mutation == "mu1_sign" else 1) * bs * np.asarray(params["mu1"], dtype=X) / (r * h)
    mum = mu * m
    dt, dt_t = np.zeros((T + 1, V), dtype=X), np.zeros((T + 1, V), dtype=X)
    dt[:-1] += mum / h
    dt[1:] -= mum / h
    if mutation == "mu0_interval":
        dt[0] -= 2 * mum[0] / h
    dt_t[:-1] += np.abs(mum) / h
    dt_t[1:] += np.abs(mum) / h
    ge = sum(hat[None, :, :, c] * E[:, :, None, c] for c in range(3)) * w[None, :, None]      # [t, f, k]
    ge_t = sum(np.abs(hat_s[None, :, :, c] * E[:, :, None, c]) for c in range(3)) * w[None, :, None]
    ge = ge.reshape(T + 1, 3 * F)
    if mutation == "odd_corner":
        ge = ge.copy()
        ge[:, last_odd] = 0
    x = bnd + dt - _gather(ge, cv, V)
    x_t = np.abs(bnd) + dt_t + _gather(ge_t.reshape(T + 1, 3 * F), cv, V)
    put("V_DUALAUX2", (r * h) * x / m, (r * h) * x_t / m, (3 * val + 12 + TAB_HAT + TAB_AREA)[None, :] + tab_m, m, tab_m, N)
    # -- Dual(beta): mu + sz (beta_end - beta_fst), E + L^T beta_mid (:484-503)
    a1 = sz * (be - bf)
    a1_t = np.abs(sz * be) + np.abs(sz * bf)
    put("V_MU2", mu, np.abs(mu), 0, m, tab_m, I,
        drop=(lambda c: c * (~np.isin(np.arange(V), numbering.last_tile_vertices()))[None, :]) if mutation == "ragged_tile" else None)
    put("V_AUX1_2", a1, a1_t, 2, m, tab_m, I)
    put("V_MUAUX1_2", mu + a1, np.abs(mu) + a1_t, 3, m, tab_m, I)
    a2, a2_t = np.zeros((T + 1, F, 3), dtype=X), np.zeros((T + 1, F, 3), dtype=X)
    a2[:-1] += c3 * bm[:, 0].sum(axis=1)
    a2[1:] += c3 * bm[:, 1].sum(axis=1)
    a2_t[:-1] += np.abs(c3 * bm[:, 0]).sum(axis=1)
    a2_t[1:] += np.abs(c3 * bm[:, 1]).sum(axis=1)
    put("F_E2", E, np.abs(E), 0, wf, TAB_AREA, N)
    put("F_AUX2_2", a2, a2_t, 8, wf, TAB_AREA, N)
    put("F_EAUX2_2", E + a2, np.abs(E) + a2_t, 9, wf, TAB_AREA, N)
    # -- Comp(rho, f(q)): aux = ps A + q / (4 m), q the corner sum of area |L(ps B)|^2; max(0, aux + rho) - rho (:505-526 with :615-619)
    rho = (ds * r) * mu
    sqn = ((ps * B) ** 2).sum(axis=2)                                        # [node, f]
    nxt = sqn[1:].copy()
    if mutation == "pair_reads_t1":
        odd = np.arange(T) % 2 == 1
        nxt[odd] = sqn[:-1][odd]
    per = np.repeat(((sqn[:-1] + nxt) * w[None, :] / 3)[:, :, None], 3, axis=2).reshape(T, 3 * F)
    q = _gather(per, cv, V)
    aux = ps * A + q / m / 4
    aux_t = np.abs(ps * A) + q / m / 4
    n_aux = (val + 13 + TAB_AREA)[None, :] + tab_m
    put("V_COMP_AUX2", aux, aux_t, n_aux, m, tab_m, I)
    put("V_COMP_RES2", np.maximum(0, aux + rho) - rho, aux_t + 2 * np.abs(rho), n_aux + 4, m, tab_m, I)
    # -- Comp(rho, cong.): cong rho - ps lambda_c (:549-559 with :633-636)
    rho_c = (ps * r) * mu if mutation == "cong_prim_scale" else rho
    put("V_CONG_RES2", cong * rho_c - ps * lc, np.abs(cong * rho) + np.abs(ps * lc), 5, m, tab_m, I)
    # -- Comp(m, rho o B): the node and triangle average of rho times ps B, minus m = ds r E (:528-547 with :624-628)
    rho_n, rho_n_t = np.zeros((T + 1, V), dtype=X), np.zeros((T + 1, V), dtype=X)
    rho_n[:-1] += rho / 2
    rho_n[1:] += rho / 2
    rho_n_t[:-1] += np.abs(rho) / 2
    rho_n_t[1:] += np.abs(rho) / 2
    rho_f = sum(rho_n[:, s.tri[:, k]] for k in range(3))[:, :, None] / 3
    rho_f_t = sum(rho_n_t[:, s.tri[:, k]] for k in range(3))[:, :, None] / 3
    aux5, aux5_t = rho_f * (ps * B), rho_f_t * np.abs(ps * B)
    put("F_AUX5_2", aux5, aux5_t, 10, wf, TAB_AREA, N)
    put("F_AUX5M_2", aux5 - (ds * r) * E, aux5_t + np.abs((ds * r) * E), 13, wf, TAB_AREA, N)

    # -- the objective's sums (:417-431 as called at :773-775): <phi[0], mu0>, <phi[T], mu1>, sum lambda_c^2 m
    obj, obj_b = np.zeros(3, dtype=X), np.zeros(3, dtype=X)
    for i, (node, dens) in enumerate(((0, "mu0"), (T - 1 if mutation == "objective_node" else T, "mu1"))):
        if n0 <= (0, T)[i] < n0 + nl:
            c = phi[node] * np.asarray(params[dens], dtype=X)
            obj[i], obj_b[i] = c.sum(), U * (1 + V) * np.abs(c).sum()
    c = (lc * lc * m)[I]
    obj[2], obj_b[2] = c.sum(), (U * (2 + tab_m) * (lc * lc * m))[I].sum() + U * c.size * c.sum()

    # -- norm_square (:875-878 with the weights of :215-218); a slab's share over the global average count
    norms, norms_b = {}, {}
    corner_w = w[None, None, None, :, None]
    for (name, part), kind in NORMS.items():
        if (name, part) == ("phi", 1):
            e, t, n, wgt, tab, rows, avg = dphi, dphi_t, 4, m, tab_m, I, T
        elif (name, part) == ("phi", 2):
            e, t, n, wgt, tab, rows, avg = gx, gx_t, 3 + TAB_HAT, wf, TAB_AREA, N, T + 1
        elif kind == 3:
            e = np.zeros((T + 1, 2, 3, F, 3), dtype=X)
            e[:-1, 0], e[1:, 1] = a[name][:, 0], a[name][:, 1]
            if mutation == "norm_extra_column":
                e[0, 1] = a[name][T - 1, 1]
            t, n, wgt, tab, rows, avg = np.abs(e), 0, corner_w, TAB_AREA, N, T
        else:
            e = a[name]
            t, n, wgt, tab, rows, avg = np.abs(e), 0, (m if kind <= 1 else wf), (tab_m if kind <= 1 else TAB_AREA), (N if kind != 1 else I), (T if kind == 1 else T + 1)
        c = e * e * wgt
        norms[(name, part)] = c[rows].sum() / avg
        if bounds:
            de = U * n * t
            b = (2 * np.abs(e) * de + de * de) * wgt + U * (2 + tab) * c
            norms_b[(name, part)] = (b[rows].sum() + U * (c[rows].size + 1) * c[rows].sum()) / avg
    return dict(kkt=sums, kkt_bound=bnd_out, objective=obj, objective_bound=obj_b, norms=norms, norms_bound=norms_b)


def reference(s, state, params, slab=None, halos=None):
    """Every KKT slot (``kkt``, in ``SLOTS`` order), the three objective sums and every norm in long double, each with its running error
    bound for an fp64 evaluation (``*_bound``).  ``s``: an oracle solver (its geometry tables and sizes are read, not its state);
    ``state``: the twelve arrays in the reference layouts; ``params``: ``params_of``.  ``slab = (first node, node count)``: the share
    of that time slab (its intervals, its nodes, the corner entries compared with its nodes); ``halos``: dict of ``mu_lo``, ``B_hi``,
    ``phi_hi`` to read in place of the neighbouring slabs' entries of ``state``."""
    return _evaluate(s, state, params, LD, True, slab=slab, halos=halos)


def plain(s, state, params, mutation=None, slab=None, halos=None, numbering=None):
    """The same sums in fp64 numpy; ``mutation``: one of ``MUTATIONS`` (``ragged_tile`` and ``neighbour_area`` read the ``numbering``)."""
    if numbering is None:
        numbering = Numbering(s.T, s.V, s.F)
    return _evaluate(s, state, params, np.float64, False, mutation=mutation, slab=slab, halos=halos, numbering=numbering)


def flat(res):
    """``(names, values, bounds)`` of everything an evaluation holds; ``bounds`` is None where it has none (``plain``)."""
    names = list(SLOTS) + ["objective." + k for k in OBJECTIVE] + [f"norm.{k}.{p}" for k, p in NORMS]
    vals = list(res["kkt"]) + list(res["objective"]) + [res["norms"][k] for k in NORMS]
    bnds = None
    if res["norms_bound"]:
        bnds = np.array(list(res["kkt_bound"]) + list(res["objective_bound"]) + [res["norms_bound"][k] for k in NORMS], dtype=LD)
    return names, np.array(vals, dtype=LD), bnds


def tolerances(ref, pl):
    """Per entry of ``flat``: MARGIN max(|plain - reference|, bound); 0 where the reference is exactly 0."""
    names, r, b = flat(ref)
    _, p, _ = flat(pl)
    tol = MARGIN * np.maximum(np.abs(p - r), b)
    return names, r, np.where(r == 0, LD(0), tol)


def ratios(got, ref, tol):
    """|got - ref| / tol per entry (where the reference is exactly 0: 0 if got is exactly 0.0, inf otherwise)."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(got == 0.0, 0.0, np.inf)).astype(np.float64)
    return q


def assert_within(got, names, ref, tol, what=""):
    q = ratios(got, ref, tol)
    bad = np.nonzero(~(q <= 1.0))[0]
    if bad.size:
        i = bad[np.argmax(np.nan_to_num(q[bad], nan=np.inf))]
        raise AssertionError(f"{what}: {names[i]}: got {float(got[i])!r}, reference {float(ref[i])!r}, |difference| / tolerance = {q[i]:.3g}"
                             f" (tolerance {float(tol[i]):.3e}); {bad.size} of {len(names)} entries miss: {[names[j] for j in bad[:8]]}")
    return float(q.max()) if q.size else 0.0


def device_vector(kkt_sums, objective_sums, norms):
    """A device's answers in the order of ``flat``."""
    return np.concatenate([np.asarray(kkt_sums, dtype=np.float64)[:N_SUMS], np.asarray(objective_sums, dtype=np.float64),
                           np.array([norms[k] for k in NORMS], dtype=np.float64)])


# ---- the link to the oracle ---------------------------------------------------------------------------------------------------------
def combine(sums, s):
    """The seven residuals from the slots, as dots_kkt_combine forms them (the closures of solver_socp.py:433-559 on sums): a list of
    [value, value at unit scale or None]."""
    q = {k: float(sums[i]) for k, i in IX.items()}
    T, T1 = float(s.T), float(s.T + 1)
    sq = lambda *t: float(np.sqrt(sum(t)))      # noqa: E731
    ps, ds, r = s.prim_scale, s.dual_scale, s.r
    pair = lambda num, const, rest, scale: [num / (const / k + rest) for k in (scale, 1.0)]      # noqa: E731
    rho2 = (ds * r) ** 2
    return [
        pair(sq(q["V_RESMU2"] / T, q["F_RESE2"] / T1), s.c_prim_q,
             sq(q["V_DPHI2"] / T, q["F_DX2"] / T1) + sq(q["V_A2"] / T, q["F_B2"] / T1) + sq(q["V_LAM2"] / T), ps),
        pair(sq(q["V_RFST2"] / T, q["V_REND2"] / T, q["F_RMID2"] / T), s.c_prim_z, s.norm_d, ps),
        pair(sq(q["V_DUALAUX2"] / T1), s.c_dual_alpha, s.norm_boundary, ds),
        pair(r * sq(q["V_MUAUX1_2"] / T, q["F_EAUX2_2"] / T1), s.c_dual_beta,
             r * (sq(q["V_MU2"] / T, q["F_E2"] / T1) + sq(q["V_AUX1_2"] / T, q["F_AUX2_2"] / T1)), ds),
        [sq(q["V_COMP_RES2"] / T) / (s.c_comp_rho + sq(rho2 * q["V_MU2"] / T) + sq(q["V_COMP_AUX2"] / T)), None],
        [sq(q["F_AUX5M_2"] / T1) / (s.c_comp_m + sq(rho2 * q["F_E2"] / T1) + sq(q["F_AUX5_2"] / T1)), None],
        [sq(q["V_CONG_RES2"] / T) / (s.c_comp_rho + sq(rho2 * q["V_MU2"] / T) + sq(ps * ps * q["V_LAM2"] / T)), None],
    ]


def oracle_kkt(s, state):
    """``OracleSolver.kkt_functions`` on ``state`` (step_checks.compare_kkt's preparation)."""
    sc.load(s, state)
    s.dt_phi = O.grad_time(s.h, s.phi)
    s.dx_phi = O.grad_space(s.G, s.F, s.phi)
    s.dec_B = O.decouple(s.B, s.sz)
    return [f() for f in s.kkt_functions()]


# ---- the states -----------------------------------------------------------------------------------------------------------------------
def white(s, seed):
    """The recipe of random_state (test_hip_phases.py)."""
    rng = np.random.default_rng(seed)
    st = {k: rng.standard_normal(getattr(s, k).shape) for k in STATE}
    st["beta_fst"][:, ::3] -= 6.0
    st["beta_fst"][:, 1::3] += 6.0
    return st


CONVERGED_K = (10, 60, 300)
PRIM, DUAL = 3.0, 0.625      # the explicit factors of scale_prim_dual: the three scales differ from 1 (boundary_scale = 1 / DUAL)


def converged(T, geom, congestion, ks=CONVERGED_K):
    """The oracle's own iterates after k iterations from its start (k in ``ks``, ascending), each followed by scale_prim_dual(PRIM, DUAL):
    a list of (s, state, params), every ``s`` a solver of its own that holds the scalars of its state."""
    import copy

    s = O.OracleSolver(T, geom, congestion=congestion)
    out, done = [], 0
    for k in ks:
        for _ in range(k - done):
            s.iterate()
        done = k
        snap = copy.copy(s)      # (shallow: the arrays are replaced, not written, by scale_prim_dual; the state is copied below)
        for name in STATE + ("bnd", "dt_phi", "dx_phi"):
            setattr(snap, name, getattr(s, name).copy())
        snap.scale_prim_dual(PRIM, DUAL)
        assert snap.prim_scale == PRIM and snap.dual_scale == DUAL
        out.append((snap, sc.snapshot(snap), params_of(snap, geom, boundary_scale=1.0 / DUAL)))
    return out


def probe_supports(s, numbering):
    """name -> (kind, index): the small supports of ``probe``; vertices and triangle rows are picked in the DEVICE numbering and given
    in the caller's."""
    T, V, F = s.T, s.V, s.F
    nb = numbering
    out = {}
    for t in sorted({0, 1, T - 1, T}):
        if 0 <= t <= T:
            out[f"time{t}"] = ("time", (t,))
    even = 2 * ((T // 2) // 2)      # an even node well inside
    out[f"pair{even}"] = ("time", (even, even + 1)) if even + 1 <= T else ("time", (even,))
    last = T - T % 2                # the last lane: nodes (T - 1, T) when T is odd, node T alone when T is even
    out[f"lastpair{last}"] = ("time", tuple(t for t in (last, last + 1) if t <= T))
    cv, val, _ = _corner_tables(s)
    edges = np.sort(np.concatenate([s.tri[:, [0, 1]], s.tri[:, [1, 2]], s.tri[:, [2, 0]]]), axis=1)
    uniq, count = np.unique(edges, axis=0, return_counts=True)
    boundary = np.unique(uniq[count == 1])
    if boundary.size:
        out["boundary_vertex"] = ("vertex", int(boundary[0]))
    if (val % 2 == 1).any():
        out["odd_valence_vertex"] = ("vertex", int(np.argmax(np.where(val % 2 == 1, val, -1))))
    VT, FT = nb.VT, nb.FT
    dv = sorted({0, min(VT, V) - 1, (nb.n_vtiles - 1) * VT, V - 1})
    for i in dv:
        out[f"device_vertex{i}"] = ("vertex", int(nb.perm_vert[i]))
    for row in sorted({(nb.n_ftiles - 1) * FT, 3 * F - 1}):
        out[f"device_row{row}"] = ("row", (int(nb.perm_tri[row // 3]), row % 3))
    return out


def probe(s, support, seed=5):
    """All twelve arrays zero except on one small support (standard normal there)."""
    rng = np.random.default_rng(seed)
    full = {k: rng.standard_normal(getattr(s, k).shape) for k in STATE}
    st = {k: np.zeros_like(v) for k, v in full.items()}
    kind, idx = support
    if kind == "time":
        for t in idx:
            for k in ("phi", "B", "E"):
                st[k][t] = full[k][t]
            if t < s.T:
                for k in STATE:
                    if k not in ("phi", "B", "E"):
                        st[k][t] = full[k][t]
    elif kind == "vertex":
        own = s.tri.T == idx                              # (3, F): the corners of the vertex
        for k in STATE:
            if k in ("z_mid", "beta_mid"):
                st[k][:, :, own] = full[k][:, :, own]
            elif k not in ("B", "E"):
                st[k][:, idx] = full[k][:, idx]
    else:
        f, c = idx
        for k in ("B", "E"):
            st[k][:, f, c] = full[k][:, f, c]
        for k in ("z_mid", "beta_mid"):
            st[k][:, :, :, f, c] = full[k][:, :, :, f, c]
    return st


def probe_params(s, geom):
    p = params_of(s, geom)
    p["const_d"] = 0.0
    return p
