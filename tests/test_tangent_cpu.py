"""Linearised transport without a GPU: the specification (tangent.velocities_host, weights_host, gram_host) against formulas written
directly, under a renumbering and through the tables a device plan holds, the plane experiment on the fp64 oracle, the drivers'
refusals before the library loads, the new entry points in header, exports and bindings, and the new kernels' resources as the
compiler reports them."""
import math
import os
import re

import numpy as np
import pytest

import flow_checks as fc
import sensitivity_checks as sc
import tangent_checks as tc
from dots_socp_amd import _lib, tangent
from dots_socp_amd.geometry import build_plan, hat_gradients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def tables(name):
    v, t = fc.mesh_of(name)
    area, hat = hat_gradients(v, t)
    return v, t, hat, area, sc.vertex_masses(v, t)


def potentials_of(name, n=3, seed=0):
    V = fc.mesh_of(name)[0].shape[0]
    rng = np.random.default_rng(4000 + seed + V)
    return rng.standard_normal((n, V)) + rng.uniform(-3.0, 3.0, (n, 1))      # (constants of size 3: no gauge is fixed)


def sigma_of(name, seed=0):
    V = fc.mesh_of(name)[0].shape[0]
    rng = np.random.default_rng(4500 + seed + V)
    sigma = 1.0 - rng.random(V)
    sigma[rng.random(V) < 0.2] = 0.0
    sigma[0] = 0.5
    return sigma


@pytest.mark.parametrize("name", sc.MESHES)
def test_the_velocities_are_the_gradient(name):
    v, t, hat, _, _ = tables(name)
    phi = potentials_of(name)
    vel = tangent.velocities_host(phi, t, hat)
    direct = np.einsum("fkc,nfk->nfc", hat, phi[:, t])
    assert vel.shape == (3, t.shape[0], 3)
    assert np.max(np.abs(vel - direct)) <= 1e-13 * np.max(np.abs(direct))
    # the stated order, as scalars, on a few triangles
    for i, f, d in ((0, 0, 0), (1, t.shape[0] - 1, 2), (2, t.shape[0] // 2, 1)):
        p = [float(phi[i][t[f][c]]) for c in range(3)]
        assert vel[i, f, d] == (float(hat[f][0][d]) * p[0] + float(hat[f][1][d]) * p[1]) + float(hat[f][2][d]) * p[2]
    # a constant of the potentials' size or more changes nothing but rounding, which is then the constant's: the shifted potentials,
    # their three products and the two sums are each within 2^-53 of |constant| max |hat| times a small count
    for constant in (3.0, -1024.0):
        shifted = tangent.velocities_host(phi + constant, t, hat)
        assert np.max(np.abs(shifted - vel)) <= 16.0 * U * abs(constant) * np.max(np.abs(hat))


@pytest.mark.parametrize("name", sc.MESHES)
def test_the_weights_sum_to_the_mass_and_the_gram_is_a_gram(name):
    v, t, hat, area, mass_v = tables(name)
    sigma = sigma_of(name)
    w = tangent.weights_host(sigma, mass_v, t, area)
    assert w.shape == (t.shape[0],) and np.all(w >= 0.0) and abs(math.fsum(w) - math.fsum(sigma)) <= 1e-14 * math.fsum(sigma)
    f = t.shape[0] - 1
    rho = [float(sigma[x]) / float(mass_v[x]) for x in t[f]]
    assert w[f] == ((rho[0] + rho[1]) + rho[2]) * (float(area[f]) * (1.0 / 3.0))
    vel = tangent.velocities_host(potentials_of(name, 5), t, hat)
    G = tangent.gram_host(vel, None, w)
    assert np.array_equal(G.view(np.int64), G.T.copy().view(np.int64))      # symmetric bit for bit
    assert np.min(np.linalg.eigvalsh(G)) >= -1e-15 * np.trace(G)
    assert G[1, 3] == math.fsum(w * ((vel[1][:, 0] * vel[3][:, 0] + vel[1][:, 1] * vel[3][:, 1]) + vel[1][:, 2] * vel[3][:, 2]))
    assert np.array_equal(tangent.gram_host(vel[:2], vel[2:], w), G[:2, 2:])
    D = tangent.squared_distances(G)
    assert np.all(D >= 0.0) and np.all(np.diag(D) == 0.0) and D[0, 1] == (G[0, 0] + G[1, 1]) - 2.0 * G[0, 1]
    assert np.array_equal(tangent.squared_distances(np.array([[1.0, 1.0 + 1e-9], [1.0 + 1e-9, 1.0]])), np.zeros((2, 2)))      # clipped


@pytest.mark.parametrize("name", sc.MESHES)
def test_the_diagonal_is_twice_the_kinetic_energy(name):
    """G_ii against sensitivity_checks.kinetic_energy_direct of a one-interval state whose phi is constant in time and whose density is
    sigma's: K = sum_f sum_k rho[v_k] (area_f / 3) |grad phi|_f^2 / 2."""
    v, t, hat, area, mass_v = tables(name)
    rho = 1.0 - np.random.default_rng(11).random(v.shape[0])
    phi = potentials_of(name, 2, seed=5)
    w = tangent.weights_host(rho * mass_v, mass_v, t, area)
    G = tangent.gram_host(tangent.velocities_host(phi, t, hat), None, w)
    for i in range(2):
        K = sc.kinetic_energy_direct(rho[None, :], np.stack([phi[i], phi[i]]), v, t)
        assert abs(G[i, i] - 2.0 * K) <= 1e-13 * abs(2.0 * K)


@pytest.mark.parametrize("name", sc.MESHES)
def test_a_renumbering_permutes_the_fields_and_keeps_the_gram(name):
    v, t, hat, area, mass_v = tables(name)
    phi, sigma = potentials_of(name, 4), sigma_of(name)
    vel, w = tangent.velocities_host(phi, t, hat), tangent.weights_host(sigma, mass_v, t, area)
    G = tangent.gram_host(vel, None, w)
    pv, pf = tc.renumbering(v.shape[0], t.shape[0])
    _, t2 = tc.renumbered(v, t, pv, pf)
    vel2 = tangent.velocities_host(phi[:, pv], t2, hat[pf])
    w2 = tangent.weights_host(sigma[pv], mass_v[pv], t2, area[pf])
    assert np.array_equal(vel2, vel[:, pf]) and np.array_equal(w2, w[pf])
    assert np.all(np.abs(tangent.gram_host(vel2, None, w2) - G) <= 2.0 * np.spacing(np.abs(G)))


@pytest.mark.parametrize("name", ("torus", "plane4"))
def test_a_plan_holds_the_callers_tables_whatever_its_numbering(name):
    """device.caller_tables: the tables of a plan that renumbers the mesh, permuted back, are the caller's triangles and -- per
    triangle, formed from its own corners in its own order -- the bits of the tables of a plan that does not; the vertex masses are
    sums over the incident triangles in the numbering's order, equal to rounding."""
    from dots_socp_amd.device import caller_tables

    geom = fc.geometry_of(name)
    plain, nd = caller_tables(build_plan(1, geom, reorder=False)), caller_tables(build_plan(1, geom, reorder="nd"))
    assert build_plan(1, geom, reorder="nd").perm_vert is not None
    for got in (plain, nd):
        assert np.array_equal(got["triangles"], geom["triangles"]) and got["triangles"].dtype == np.int32
        assert got["hat"].shape == (geom["triangles"].shape[0], 3, 3)
    assert np.array_equal(nd["hat"], plain["hat"]) and np.array_equal(nd["area"], plain["area"])
    assert np.all(np.abs(nd["mass"] - plain["mass"]) <= 4.0 * np.spacing(plain["mass"]))
    area, hat = hat_gradients(geom["vertices"], geom["triangles"])
    assert np.allclose(plain["hat"], hat, rtol=1e-12, atol=1e-12) and np.allclose(plain["area"], area, rtol=1e-13)


def test_input_refusals():
    v, t, hat, area, mass_v = tables("plane4")
    phi, sigma = potentials_of("plane4"), sigma_of("plane4")
    with pytest.raises(ValueError, match="potentials must have shape"):
        tangent.velocities_host(phi[0], t, hat)
    with pytest.raises(ValueError, match="hat must have shape"):
        tangent.velocities_host(phi, t, hat[:-1])
    with pytest.raises(ValueError, match="triangle index outside"):
        tangent.velocities_host(phi[:, :-1], t, hat)
    with pytest.raises(ValueError, match="triangles must be integers"):
        tangent.velocities_host(phi, t.astype(np.float64), hat)
    with pytest.raises(ValueError, match="sigma and mass_v"):
        tangent.weights_host(sigma, mass_v[:-1], t, area)
    with pytest.raises(ValueError, match="area_f must have shape"):
        tangent.weights_host(sigma, mass_v, t, area[:-1])
    vel, w = tangent.velocities_host(phi, t, hat), tangent.weights_host(sigma, mass_v, t, area)
    with pytest.raises(ValueError, match="A must have shape"):
        tangent.gram_host(vel[0], None, w)
    with pytest.raises(ValueError, match="B must have shape"):
        tangent.gram_host(vel, vel[:, :-1], w)
    with pytest.raises(ValueError, match="w must have shape"):
        tangent.gram_host(vel, None, w[:-1])
    with pytest.raises(ValueError, match="G must be square"):
        tangent.squared_distances(np.zeros((2, 3)))
    # the measures: barycenter.check_measures in groups, with no limit on their number
    V = v.shape[0]
    many = [np.roll(np.linspace(1.0, 2.0, V), k) for k in range(40)]
    ref, m, mass = tangent.check_embedding("x", many[0], many, V)
    assert m.shape == (40, V) and mass == math.fsum(many[0])
    with pytest.raises(ValueError, match="one positive total mass"):
        tangent.check_embedding("x", many[0], many[:39] + [2.0 * many[39]], V)
    with pytest.raises(ValueError, match="negative or not finite"):
        tangent.check_embedding("x", -many[0], many, V)
    with pytest.raises(ValueError, match="reference must have shape"):
        tangent.check_embedding("x", many[0][:-1], many, V)
    with pytest.raises(ValueError, match="reference must have shape"):
        tangent.check_embedding("x", many[0], [], V)


def test_the_loop_over_a_scripted_solver():
    """tangent_embedding_host: one solve per measure from the reference, v = +grad phi0, the tables it is given."""
    v, t, hat, area, mass_v = tables("plane4")
    V = v.shape[0]
    sigma = np.full(V, 1.0 / V)
    measures = [np.roll(np.linspace(1.0, 2.0, V), k) / math.fsum(np.linspace(1.0, 2.0, V)) for k in range(3)]
    calls = []

    def solve(ref, mu):
        calls.append((ref.copy(), mu.copy()))
        k = len(calls)
        return 0.5 * k * k, k * v[:, 0] + 7.0      # phi = k x + const: the velocity (k, 0, 0), the cost k^2 / 2 for mass 1
    r = tangent.tangent_embedding_host(solve, sigma, measures, {"vertices": v, "triangles": t}, hat=hat, area_triangles=area, mass_vertices=mass_v)
    assert len(calls) == 3 and all(np.array_equal(c[0], sigma) for c in calls) and all(np.array_equal(c[1], m) for c, m in zip(calls, measures))
    assert np.allclose(r["velocities"][1], [2.0, 0.0, 0.0], atol=1e-12) and np.array_equal(r["costs"], [0.5, 2.0, 4.5])
    assert np.allclose(r["gram"], np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]), rtol=1e-12)
    assert np.allclose(r["squared_distances"][0, 2], 4.0, rtol=1e-11)
    own = tangent.tangent_embedding_host(lambda ref, mu: (0.5, v[:, 1]), sigma, measures[:1], {"vertices": v, "triangles": t})      # its own tables
    assert abs(own["gram"][0, 0] - 1.0) <= 1e-12 and np.allclose(own["weights"], r["weights"], rtol=1e-13)


# ---- the plane experiment on the fp64 oracle --------------------------------------------------------------------------------------------
def test_the_linearisation_holds_on_the_oracle():
    """Four Gaussians seen from a fifth on the plane (V = 132, F = 220, T = 7, tol 1e-5), six oracle solves, about 6 s.  Measured:
    G_ii / (2 cost_i) = 1.0026, 1.0025, 1.0026, 1.0026 (an O(h) gap); |v_i - v_j|^2 against twice the direct cost of the pairs (0, 1)
    and (2, 3): 3.3e-4 and 1.4e-4 relative; the sigma-weighted mean velocity against the displacement: 5.2e-4."""
    geom, sigma, measures, moves = tc.plane_case()
    assert geom["vertices"].shape[0] == 132 and geom["triangles"].shape[0] == 220
    solve = tc.oracle_solve(geom)
    r = tangent.tangent_embedding_host(solve, sigma, measures, geom)
    pair_costs = {(i, j): float(solve(measures[i], measures[j])[0]) for i, j in tc.PLANE_PAIRS}
    own, pairs, mean = tc.plane_figures(r["gram"], r["costs"], r["velocities"], r["weights"], moves, pair_costs)
    continuum = moves @ moves.T
    print("G_ii / (2 cost_i)", [float(r["gram"][i, i] / (2.0 * r["costs"][i])) for i in range(4)], "max |G - d_i . d_j|",
          float(np.max(np.abs(r["gram"] - continuum))), "pairs", pairs, "mean velocity", mean)
    assert own <= tc.BOUND_SELF
    assert max(pairs) <= tc.BOUND_PAIR
    assert mean <= tc.BOUND_MEAN      # (so the sign is v = +grad phi0)
    assert abs(math.fsum(r["weights"]) - 1.0) <= 1e-13


# ---- the drivers' refusals, before the library ------------------------------------------------------------------------------------------
def test_the_drivers_refuse_before_the_library(monkeypatch):
    from dots_socp_amd import socp

    def refuse(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)
    geom, sigma, measures, _ = tc.plane_case()
    for call in (lambda **kw: socp.tangent_embedding(7, geom, sigma, measures, **kw), lambda **kw: socp.distance_matrix(7, geom, measures, **kw)):
        with pytest.raises(ValueError, match="time slabs"):
            call(time_slab=(0, 2))
        with pytest.raises(ValueError, match="is_constant_scaling"):
            call(is_constant_scaling=True)
        with pytest.raises(ValueError, match="unknown option"):
            call(preconditioner="jacobi")
    with pytest.raises(ValueError, match="reference must have shape"):
        socp.tangent_embedding(7, geom, sigma[:-1], measures)
    with pytest.raises(ValueError, match="reference must have shape"):
        socp.tangent_embedding(7, geom, sigma, [measures[0][:-1]])
    with pytest.raises(ValueError, match="one positive total mass"):
        socp.tangent_embedding(7, geom, 2.0 * sigma, measures)
    with pytest.raises(ValueError, match="negative or not finite"):
        socp.tangent_embedding(7, geom, sigma, [measures[0], np.where(np.arange(sigma.shape[0]) == 3, np.nan, measures[1])])
    with pytest.raises(ValueError, match="geometry must be a dict"):
        socp.tangent_embedding(7, {"vertices": geom["vertices"]}, sigma, measures)
    with pytest.raises(ValueError, match="method must be"):
        socp.distance_matrix(7, geom, measures, method="exact")
    with pytest.raises(ValueError, match="takes no reference"):
        socp.distance_matrix(7, geom, measures, method="pairs", reference=sigma)
    with pytest.raises(ValueError, match="one positive total mass"):
        socp.distance_matrix(7, geom, [measures[0], 3.0 * measures[1]])


# ---- the build ----------------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("dots_tangent_velocities", "dots_tangent_weights", "dots_tangent_gram_scratch", "dots_tangent_gram")


def test_header_exports_and_version_agree_on_the_new_entries():
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(dots_[a-z_0-9]+)\s*\(", code))
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and name in names
        assert not re.search(r"%s\((?:const )?dots_ctx \*" % name, code)      # the calls take no context: admission.h keeps its rows
    assert re.search(r"#define\s+DOTS_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7      # additions: the ABI version stays
    assert "typedef struct dots_tangent_desc" in code
    with open(os.path.join(ROOT, "dots_socp_amd", "csrc", "exports.map")) as fh:
        assert "dots_*" in fh.read()      # the C ABI is listed by its prefix
    from dots_socp_amd import build

    assert "kernels_tangent.hip" in build.SOURCES and any(h.endswith("pairs_dev.h") for h in build.HEADERS)


def test_the_descriptor_matches_the_header(tmp_path):
    import ctypes

    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(dots_tangent_desc), offsetof(dots_tangent_desc, triangles), offsetof(dots_tangent_desc, mass_vert), "
                   "offsetof(dots_tangent_desc, stream), offsetof(dots_tangent_desc, ms)); return 0;}\n")
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    D = _lib.TangentDesc
    assert got == [ctypes.sizeof(D), D.triangles.offset, D.mass_vert.offset, D.stream.offset, D.ms.offset]


def test_the_library_refuses_bad_sizes_on_the_host():
    """dots_tangent_gram_scratch is host arithmetic: (2 chunks + 1) na nb doubles, chunks = ceil(F / 2048) up to 1024."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library is not built")
    lib = _lib.load(host_only=True)
    assert lib.dots_tangent_gram_scratch(3, 5, 220) == 3 * 15 and lib.dots_tangent_gram_scratch(17, 17, 2080) == 5 * 289
    assert lib.dots_tangent_gram_scratch(1, 1, 2048) == 3 and lib.dots_tangent_gram_scratch(1, 1, 2049) == 5
    assert lib.dots_tangent_gram_scratch(2, 2, 2048 * 5000) == (2 * 1024 + 1) * 4
    for bad in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (-1, 1, 4), (4097, 1, 4), (1, 4097, 4)):
        assert lib.dots_tangent_gram_scratch(*bad) == -1


def test_the_new_kernels_need_no_scratch(tmp_path):
    """k_tangent_*: no private segment and no spills, from the code object's metadata (as test_kernel_resources_cpu.py reads it)."""
    import test_kernel_resources_cpu as kr

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library is not built")
    if not kr.READELF or not kr.OBJCOPY:
        pytest.skip("llvm-readelf / llvm-objcopy not found")
    records = [r for co in kr.code_objects(_lib.LIB_PATH, str(tmp_path)) for r in kr.kernel_records(co)]
    mine = {kr.short_name(r["name"]): r for r in records if kr.short_name(r["name"]).startswith("k_tangent")}
    assert sorted(mine) == ["k_tangent_gram", "k_tangent_gram_fold", "k_tangent_velocities", "k_tangent_weights"]
    for name, r in mine.items():
        assert int(r["private_segment_fixed_size"]) == 0 and int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, (name, r)
        assert int(r["max_flat_workgroup_size"]) == 256, (name, r)
    assert int(mine["k_tangent_gram"]["group_segment_fixed_size"]) == 1024      # 16 entries x 4 waves x (hi, lo)
    assert all(int(mine[k]["group_segment_fixed_size"]) == 0 for k in mine if k != "k_tangent_gram")
