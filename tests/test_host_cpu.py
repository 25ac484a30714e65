"""CPU tests (no GPU): the C-ABI library loads and exports every symbol the header declares, the
host control logic takes the same decisions as the oracle's restatement of the reference, and the
host-side operator assembly matches the oracle's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN_DIR, ROOT, has_gpu, load_oracle

O = load_oracle()


# ---------------------------------------------------------------------------- C ABI
def header_functions():
    text = open(os.path.join(ROOT, "include", "dots_socp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dots_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from dots_socp_amd import _lib

    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
    assert set(_lib.EXPORTS) == set(names)
    assert lib.dots_abi_version() == _lib.ABI_VERSION


def test_library_exports_nothing_but_the_header():
    """The header is the ABI: the dynamic symbol table of the library holds the declared entry points and nothing else
    (-fvisibility=hidden + csrc/exports.map; no C++ internals, no kernel stubs)."""
    import subprocess

    from dots_socp_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == header_functions()


def test_struct_layouts_match_the_header(tmp_path):
    """Compile a probe with gcc against the header and compare sizes/offsets with the ctypes mirror."""
    from dots_socp_amd import _lib

    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
        "int main(void){printf(\"%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(dots_problem_desc), sizeof(dots_params),"
        " sizeof(dots_step_stats), sizeof(dots_mg_level), sizeof(dots_mg_desc), offsetof(dots_params, cg_tol),"
        " offsetof(dots_mg_level, ap_val_p), sizeof(dots_front_desc), offsetof(dots_front_desc, values),"
        " sizeof(dots_penalty_policy), offsetof(dots_penalty_policy, factor)); return 0;}\n"
    )
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    out = os.popen(str(exe)).read().split()
    want = [ctypes.sizeof(_lib.ProblemDesc), ctypes.sizeof(_lib.Params), ctypes.sizeof(_lib.StepStats),
            ctypes.sizeof(_lib.MgLevel), ctypes.sizeof(_lib.MgDesc), _lib.Params.cg_tol.offset, _lib.MgLevel.ap_val_p.offset,
            ctypes.sizeof(_lib.FrontDesc), _lib.FrontDesc.values.offset, ctypes.sizeof(_lib.PenaltyPolicy), _lib.PenaltyPolicy.factor.offset]
    assert [int(x) for x in out] == want


@pytest.mark.skipif(has_gpu(), reason="checks the failure mode on a machine without a GPU")
def test_no_silent_cpu_fallback():
    from dots_socp_amd import _lib, meshes
    from dots_socp_amd.socp import solver_socp

    geom, _ = meshes.example("sphere", level=1)
    with pytest.raises(_lib.HipLibraryError):
        solver_socp(4, geom, nit=1)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dots_socp_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "dots_oracle" not in text and "oracle/" not in text.replace("the oracle", ""), f


# ---------------------------------------------------------------------------- control logic
def test_penalty_policy_matches_oracle():
    from dots_socp_amd.control import AdjustAdmmParam

    a, b = AdjustAdmmParam(), O.PenaltyPolicy()
    hits = []
    for it in range(1200):
        x, y = a.is_to_adjust(it), b.is_to_adjust(it)
        assert x == y
        if x:
            hits.append(it)
    assert hits[:8] == [2, 5, 8, 11, 14, 17, 24, 31]        # schedule of admm_tools.py:43-48
    for gap in np.concatenate([np.logspace(-3, 3, 200), [1.0, 1.2, 1.5, 2, 2.5, 3, 5, 10, 20, 35, 50]]):
        assert AdjustAdmmParam.adjust_factor(gap) == O.PenaltyPolicy.factor(gap)
        assert a.get_updated_value(0.7, gap) == b.updated(0.7, gap)
    assert a.get_updated_value(900.0, 100.0) == 1000.0 and a.get_updated_value(1.5e-3, 1e-3) == 1e-3
    nan = float("nan")
    for row in ([1e-3, 2e-3, 1e-4], [nan, 1e-3, 1e-3], [1e-3, nan, 1e-3], [6e-3, 1e-3, 1e-3]):
        p, q = AdjustAdmmParam(), O.PenaltyPolicy()
        assert p.is_to_scale_matrix(150, row) == q.is_to_rescale_z(150, row)
        assert p.is_to_scale_matrix(50, row) is False
    assert [it for it in range(400) if AdjustAdmmParam.is_to_scale(it)] == [10, 50, 150, 250, 350]


def test_error_condition_swallows_arithmetic_but_not_library_errors():
    """control.ErrorCondition: an arithmetic failure of the evaluation reads as inf / not passed (the reference's
    behaviour, condition_validator.py:140-150); a library error (device fault, stale z_mid) propagates."""
    from dots_socp_amd._lib import HipLibraryError
    from dots_socp_amd.control import ErrorCondition

    def zero_div():
        return [1.0 / 0.0, None]

    c = ErrorCondition(zero_div, 1e-3, "x")
    assert c() is False and c.take() == [float("inf"), float("inf")]

    def broken():
        raise HipLibraryError("dots_kkt failed with status -5")

    with pytest.raises(HipLibraryError):
        ErrorCondition(broken, 1e-3, "y")()


def _drive_validators(seed, n_iter=400, tol=1e-3):
    """Feed the same synthetic error streams to both implementations and compare every decision."""
    from dots_socp_amd.control import AdaptiveValidator, AdjustAdmmParam, ConditionValidator, ErrorCondition, max_of_list_with_none

    rng = np.random.default_rng(seed)
    base = 10.0 ** rng.uniform(-1.0, 0.5, size=7)
    decay = rng.uniform(0.97, 0.995, size=7)
    state = {"it": 0}

    def err(i):
        e = base[i] * decay[i] ** state["it"] * (1.0 + 0.3 * np.sin(0.37 * state["it"] + i))
        return [float(e), float(e) if i < 4 else None]

    mine = AdaptiveValidator(ConditionValidator([ErrorCondition((lambda i=i: err(i)), tol, str(i)) for i in range(7)],
                                                [6, 2, 0, 3, 1, 4, 5]))
    theirs = O.LazyKKT([(lambda i=i: err(i)) for i in range(7)], tol, order=[6, 2, 0, 3, 1, 4, 5])
    pa, pb = AdjustAdmmParam(), O.PenaltyPolicy()
    log = []
    for it in range(n_iter):
        state["it"] = it
        adjust = pa.is_to_adjust(it)
        assert adjust == pb.is_to_adjust(it)
        req = [0, 1, 2, 3] if adjust else None
        if adjust:
            mine.reset_counter()
            theirs.reset_counter()
        p1, _ = mine.validate(req)
        p2, _ = theirs.validate(req)
        o1, s1 = mine.collect()
        o2, s2 = theirs.collect()
        if adjust:
            mine.reset_counter()
            theirs.reset_counter()
        assert p1 == p2 and o1 == o2 and s1 == s2, it
        e = max_of_list_with_none([o1[i] for i in (0, 2, 4, 5)])
        if e is not None:
            mine.set_error_and_tolerance(e, tol)
            theirs.set_error(e, tol)
        log.append([i for i, v in enumerate(o1) if v is not None])
        if p1:
            break
    return log


@pytest.mark.parametrize("seed", range(6))
def test_lazy_validator_matches_oracle(seed):
    log = _drive_validators(seed)
    assert any(len(x) == 0 for x in log) and any(len(x) >= 4 for x in log)   # both skipped and required rounds occur


def test_running_history_record_semantics():
    from dots_socp_amd.control import RunningHistory

    h = RunningHistory(5)
    h.start()
    assert np.all(np.isinf(h.get_current_kkt_errors()))
    h.record(0, [1, None, 2, None, None, None, None])
    h.record(1, [None] * 7)
    h.record(1, [3, 3, 3, 3, 3, 3, 3], history={"Transportation cost": 0.5})     # same iteration: overwrite
    h.end()
    assert h.kkt_errors.shape == (2, 7) and np.isnan(h.kkt_errors[0, 1]) and h.kkt_errors[1, 0] == 3
    assert h.kkt_iteration.tolist() == [0, 1] and h.history["Transportation cost"].tolist() == [np.inf, 0.5]
    with pytest.raises(ValueError):
        h.record(0, [0] * 7)


# ---------------------------------------------------------------------------- assembly
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("mesh", ["sphere", "torus", "plane", "knot"])
def test_plan_matches_oracle_assembly(mesh, reorder):
    from dots_socp_amd import geometry, meshes

    kw = dict(sphere=dict(level=2), torus=dict(nu=14, nv=9), plane=dict(n=7), knot=dict(nu=40, nv=6))[mesh]
    geom, _ = meshes.example(mesh, **kw)
    T = 5
    plan = geometry.build_plan(T, geom, reorder=reorder)
    s = O.OracleSolver(T, geom)
    pv = plan.perm_vert if reorder else np.arange(s.V)
    pf = plan.perm_tri if reorder else np.arange(s.F)
    assert sorted(pv.tolist()) == list(range(s.V)) and sorted(pf.tolist()) == list(range(s.F))
    assert np.array_equal(pv[plan.triangles], np.asarray(geom["triangles"])[pf])
    K = sp.csr_matrix((plan.lap_val, plan.lap_col, plan.lap_rowptr), shape=(s.V, s.V))
    want = (-s.L)[pv][:, pv]
    assert abs(K - want).max() < 1e-12 * abs(want).max()          # K = G^T diag(area) G = -cot Laplacian
    assert np.allclose(plan.mass_vert, s.mass_v[pv], rtol=1e-14)
    assert np.allclose(plan.area_tri, s.area_f[pf], rtol=1e-14)
    assert np.allclose(plan.hat_grad, s.hat[pf], rtol=1e-12, atol=1e-12)
    assert np.allclose(plan.mu0, np.asarray(geom["mu0"])[pv]) and np.allclose(plan.mu1, np.asarray(geom["mu1"])[pv])
    # corner lists: every corner exactly once, under the vertex it belongs to
    assert plan.corner_ptr[0] == 0 and plan.corner_ptr[-1] == 3 * s.F
    owner = np.repeat(np.arange(s.V), np.diff(plan.corner_ptr))
    assert np.array_equal(plan.triangles.reshape(-1)[plan.corner_idx], owner)
    assert sorted(plan.corner_idx.tolist()) == list(range(3 * s.F))
    # time modes diagonalise the reference's Neumann matrix
    Q, sig = plan.time_modes, plan.time_eigs
    Lt = O.time_neumann_laplacian(T, 1.0 / T)
    assert np.max(np.abs(Q.T @ (-Lt) @ Q - np.diag(sig))) < 1e-10 and np.max(np.abs(Q.T @ Q - np.eye(T + 1))) < 1e-13
    assert np.allclose(np.sort(sig), np.sort(-s.lap_inv.eigval))


def test_plan_rejects_bad_input():
    from dots_socp_amd import geometry, meshes

    geom, _ = meshes.example("sphere", level=1)
    bad = dict(geom)
    bad["triangles"] = np.asarray(geom["triangles"]).copy()
    bad["triangles"][0, 0] = 10 ** 6
    with pytest.raises(ValueError):
        geometry.build_plan(4, bad)
    bad = dict(geom)
    bad["mu0"] = np.ones(3)
    with pytest.raises(ValueError):
        geometry.build_plan(4, bad)
    bad = dict(geom)
    bad["triangles"] = np.asarray(geom["triangles"]).copy()
    bad["triangles"][0] = [0, 0, 1]          # degenerate triangle
    with pytest.raises(ValueError):
        geometry.build_plan(4, bad, reorder=False)


def test_mesh_generators():
    from dots_socp_amd import meshes

    for (v, t), chi in ((meshes.icosphere(3), 2), (meshes.torus(20, 12), 0), (meshes.torus_knot_tube(2, 5, 48, 8), 0),
                        (meshes.plane(9), 1)):
        e = meshes._unique_edges(t)
        assert v.shape[0] - e.shape[0] + t.shape[0] == chi
        assert np.all(meshes.triangle_areas(v, t) > 0) and np.unique(t).size == v.shape[0]
    g, scale = meshes.example("sphere", level=2)
    assert abs(g["mu0"].sum() - 1) < 1e-14 and abs(g["mu1"].sum() - 1) < 1e-14
    assert np.allclose(g["vertices"].min(0), 0) and abs(g["vertices"].max() - 1) < 1e-14 and scale == pytest.approx(0.5)
    assert meshes.icosphere(5)[0].shape[0] == 10242 and meshes.torus(400, 250)[0].shape[0] == 100000


def test_evaluate_helpers_match_the_reference_outputs():
    """dots_socp_amd/evaluate.py against the outputs of the reference's utils/evaluate_solution.py:7-58 (and its
    utils/util.py:32-67 norms) recorded by tests/golden/make_golden.py f1 on two recorded solutions."""
    from dots_socp_amd import evaluate, meshes

    for fname in ("f1_ico2_T15_ckpt.npz", "f1_torus_T7_cong.npz"):
        g = np.load(os.path.join(GOLDEN_DIR, fname))
        at = meshes.triangle_areas(g["vertices"], g["triangles"])
        geom = {"area_vertices": meshes.vertex_areas(g["vertices"].shape[0], g["triangles"], at)}
        for tag in ("raw", "center"):
            mu, exact = g[f"{tag}_mu"], g[f"{tag}_exact"]
            got = evaluate.check_mass_conservation(mu)
            assert isinstance(got, float) and abs(got - float(g[f"{tag}_mass_conservation"])) <= 1e-14 * max(1.0, abs(got))
            err, layers = evaluate.check_negative_mass(mu)
            assert abs(err - float(g[f"{tag}_negative_mass"])) <= 1e-14 * max(1e-30, abs(err)) + 1e-300
            assert np.allclose(layers, g[f"{tag}_negative_mass_layers"], rtol=1e-13, atol=0)
            d = evaluate.compare_with_exact_transportation(mu, exact, geom)
            assert np.allclose([d["l1"], d["l2"], d["linf"]], g[f"{tag}_versus_exact"], rtol=1e-12, atol=0), (fname, tag)
    # 1-D input: no time step in the norms (utils/util.py:35-39, 51-55)
    w = geom["area_vertices"] / 3.0
    d = evaluate.compare_with_exact_transportation(mu[3], exact[3], geom)
    rho, rho_x = mu[3] / w, exact[3] / w
    assert abs(d["l1"] - np.sum(np.abs(rho - rho_x) * w) / (1.0 + np.sum(np.abs(rho_x) * w))) < 1e-15
    assert abs(d["l2"] - np.sqrt(np.sum((rho - rho_x) ** 2 * w)) / (1.0 + np.sqrt(np.sum(rho_x ** 2 * w)))) < 1e-15


def test_plane_exact_transport_matches_the_reference():
    """evaluate.plane_exact_transportation against data/settings/plane.py:29-46 (recorded un-normalised masses)."""
    from dots_socp_amd import evaluate

    g = np.load(os.path.join(GOLDEN_DIR, "f1_plane_exact.npz"))
    got = evaluate.plane_exact_transportation(g["t_array"], g["vertices"], g["area_vertices"])
    want = g["exact"] / g["exact"].sum(axis=1, keepdims=True)        # every layer normalised to mass 1 here
    assert np.allclose(got, want, rtol=1e-12, atol=1e-300)


def test_example_settings_match_the_reference_get_mu():
    """dots_socp_amd/examples.py against get_mu of every data/settings/*.py (recorded on synthetic meshes)."""
    from dots_socp_amd import examples

    g = np.load(os.path.join(GOLDEN_DIR, "settings_get_mu.npz"))
    names = sorted({k[:-4] for k in g.files if k.endswith("_mu0") and not k.startswith("sphere_")})
    assert set(names) == set(examples.RECIPES) and len(names) == 22
    for mesh, cases in (("", names), ("sphere_", ["eight", "knots_3"])):
        v, av = g[mesh + "vertices"], g[mesh + "area_vertices"]
        for n in cases:
            m0, m1 = examples.get_mu(n, av, v)
            for got, want in ((m0, g[f"{mesh}{n}_mu0"]), (m1, g[f"{mesh}{n}_mu1"])):
                assert np.max(np.abs(got - want)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300), (mesh, n)
    with pytest.raises(ValueError):
        examples.get_mu("no_such_example", av, v)
    with pytest.raises(ValueError):
        examples.get_mu("sphere", av, v)


def test_load_example_normalises_like_the_reference(tmp_path):
    """examples.load_example: densities on the original coordinates, unit mass, unit box (load_example.py:126-139,
    data_preprocessing.py:10-17 -- normalize_geometry itself is PARITY UNPINNED: trimesh is absent here, the test
    uses its closed form (v - min) / max extent)."""
    from dots_socp_amd import examples, meshes

    v, t = meshes.torus(24, 16)
    v = 0.7 * v + np.array([0.3, -0.2, 0.1])
    path = tmp_path / "ring.off"
    meshes.write_off(path, v, t)
    geom, scale = examples.load_example("ring", str(path))
    ext = (v.max(axis=0) - v.min(axis=0)).max()
    assert abs(scale - 1.0 / ext) < 1e-15
    assert np.allclose(geom["vertices"], (v - v.min(axis=0)) / ext, rtol=0, atol=1e-15)
    av = meshes.vertex_areas(v.shape[0], t, meshes.triangle_areas(v, t))
    m0, m1 = examples.get_mu("ring", av, v)
    assert np.allclose(geom["mu0"], m0 / m0.sum(), rtol=1e-14) and np.allclose(geom["mu1"], m1 / m1.sum(), rtol=1e-14)
    assert abs(geom["mu0"].sum() - 1) < 1e-14 and abs(geom["mu1"].sum() - 1) < 1e-14


def test_off_reader_round_trip_and_errors(tmp_path):
    """meshes.read_off: contract of the reference's reader (data/util.py:73-144)."""
    from dots_socp_amd import meshes

    v, t = meshes.icosphere(1)
    path = tmp_path / "ico.off"
    meshes.write_off(path, v, t)
    text = path.read_text().replace("\n3 ", "\n\n3 ", 1)        # an empty line is skipped
    path.write_text(text)
    v2, t2, e2 = meshes.read_off(str(path))
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    assert e2.shape == (3 * t.shape[0], 2)
    assert np.array_equal(e2[:3], [[t[0, 0], t[0, 1]], [t[0, 1], t[0, 2]], [t[0, 2], t[0, 0]]])
    g, _ = meshes.make_geometry(v2, t2)
    assert g["vertices"].shape == v.shape
    for bad in ("PLY\n1 0 0\n0 0 0\n", "OFF\n", "OFF\n2 1 0\n0 0 0\n3 0 0 0\n", "OFF\n1 2 0\n0 0 0\n3 0 0 0\n", "OFF\n1 0 0\n0 0\n"):
        path.write_text(bad)
        with pytest.raises(ValueError, match="Error reading .off file"):
            meshes.read_off(str(path))
    with pytest.raises(ValueError, match="Error reading .off file"):
        meshes.read_off(str(tmp_path / "missing.off"))


def test_environment_switches_are_validated(monkeypatch):
    """DOTS_* switches are measurement aids: an unknown NAME or a value outside a switch's domain is an error, never a silent
    default."""
    from dots_socp_amd import _lib, frontal

    monkeypatch.setenv("DOTS_FRONT_VEC", "0")               # a typo of DOTS_FRONT_VEC2
    with pytest.raises(_lib.HipLibraryError, match="DOTS_FRONT_VEC"):
        _lib.check_environment()
    monkeypatch.delenv("DOTS_FRONT_VEC")
    _lib.check_environment()
    monkeypatch.setenv("DOTS_RHS_AHEAD", "yes")
    with pytest.raises(_lib.HipLibraryError, match="DOTS_RHS_AHEAD"):
        _lib.env_choice("DOTS_RHS_AHEAD", ("0", "1", "2"), "1")
    monkeypatch.setenv("DOTS_TIME_EVERY", "0")
    with pytest.raises(_lib.HipLibraryError, match="DOTS_TIME_EVERY"):
        _lib.env_choice("DOTS_TIME_EVERY", None, "32", integer=(1, 1 << 20))
    monkeypatch.setenv("DOTS_TIME_EVERY", "16")
    assert _lib.env_choice("DOTS_TIME_EVERY", None, "32", integer=(1, 1 << 20)) == "16"
    # the switches the library reads itself are checked by dots_create / dots_tree_build (host code: no GPU needed for the latter)
    lib = _lib.load()
    import ctypes as C

    monkeypatch.setenv("DOTS_ND_PCA_MIN", "many")
    indptr, indices = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    xyz = np.zeros((2, 3))
    h = C.c_void_p()
    rc = lib.dots_tree_build(2, indptr.ctypes.data_as(C.POINTER(C.c_int32)), indices.ctypes.data_as(C.POINTER(C.c_int32)),
                             xyz.ctypes.data_as(C.POINTER(C.c_double)), 4, C.byref(h))
    assert rc != 0 and b"DOTS_ND_PCA_MIN" in lib.dots_last_error()
    monkeypatch.delenv("DOTS_ND_PCA_MIN")
    # band cuts / top inverse given as arguments or through the environment
    monkeypatch.setenv("DOTS_FRONT_TOPINV", "maybe")
    with pytest.raises(_lib.HipLibraryError, match="DOTS_FRONT_TOPINV"):
        frontal.plan_bands(None, None, None, 32) if False else _lib.env_choice("DOTS_FRONT_TOPINV", ("auto", "0", "1"), "auto")


ENV_READ = re.compile(r"""(?:env_int|getenv|env_choice|os\.environ\.get)\(\s*"(DOTS_[A-Z0-9_]+)"|os\.environ\["(DOTS_[A-Z0-9_]+)"\]""")


def test_known_switches_are_the_ones_the_code_reads_and_the_ones_documented():
    """_lib.KNOWN_ENV is exactly the set of DOTS_* switches the package (Python and native code) and bench.py read, and every
    one of them has exactly one row in INTEGRATION.md's switch table."""
    import glob

    from dots_socp_amd import _lib

    pkg = os.path.join(ROOT, "dots_socp_amd")
    files = glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True) + glob.glob(os.path.join(pkg, "csrc", "*"))
    files = [f for f in files if os.path.splitext(f)[1] in (".py", ".hip", ".h")] + [os.path.join(ROOT, "bench.py")]
    read = set()
    for f in files:
        with open(f) as fh:
            read |= {a or b for a, b in ENV_READ.findall(fh.read())}
    assert read == _lib.KNOWN_ENV
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("| variable | default |"):]
    rows = [line for line in table.splitlines() if line.startswith("| `DOTS_")]
    for name in _lib.KNOWN_ENV:
        assert sum(line.startswith(f"| `{name}`") for line in rows) == 1, name
    assert len(rows) == len(_lib.KNOWN_ENV)


@pytest.mark.parametrize("name, value", [("DOTS_RHS_TILES", "0"), ("DOTS_QL_TWO", "1"), ("DOTS_CARRY", "1"), ("DOTS_CARRY_MIN", "0")])
def test_retired_switches_are_refused(monkeypatch, name, value):
    """A retired A/B switch is an unknown name: a script that still sets it fails instead of quietly measuring the default."""
    from dots_socp_amd import _lib

    monkeypatch.setenv(name, value)
    with pytest.raises(_lib.HipLibraryError, match=name):
        _lib.check_environment()


def test_device_and_pinned_memory_have_one_owner_each():
    """Over csrc/*.hip and dots_dev.h: device memory is allocated and freed inside struct DevicePool only, pinned host memory inside
    struct PinnedPool only, and the mechanisms they replaced (a context copied by value, the fixed allocation tables, the holders of
    shared and temporary buffers) are gone."""
    import glob

    csrc = os.path.join(ROOT, "dots_socp_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip"))) + [os.path.join(csrc, "dots_dev.h")]
    assert len(files) > 10
    text = {f: open(f).read() for f in files}

    def cut_struct(source, name):      # (source without the struct's body, the body)
        start = source.index(f"struct {name} {{")
        at, depth = source.index("{", start), 0
        for end in range(at, len(source)):
            depth += {"{": 1, "}": -1}.get(source[end], 0)
            if depth == 0:
                return source[:at] + source[end + 1:], source[at:end + 1]
        raise AssertionError(f"struct {name} does not close")

    header = os.path.join(csrc, "dots_dev.h")
    text[header], device_pool = cut_struct(text[header], "DevicePool")
    text[header], pinned_pool = cut_struct(text[header], "PinnedPool")
    assert device_pool.count("hipMalloc(") == 1 and device_pool.count("hipFree(") == 1
    assert pinned_pool.count("hipHostMalloc(") == 1 and pinned_pool.count("hipHostFree(") == 1
    assert "hipMalloc(" not in pinned_pool and "hipHostMalloc(" not in device_pool
    for f, source in text.items():
        for gone in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "Ctx tmp", "allocs[", "FrontStore", "DevTemps"):
            assert gone not in source, (os.path.basename(f), gone)


def test_plan_from_the_numpy_reference_functions_equals_the_native_one():
    """geometry.build_plan(native=False) (what host-only tools and the fake device of the gloo tests use: no library needed)
    gives the arrays of the library's dots_assemble."""
    from dots_socp_amd import geometry, meshes

    geom, _ = meshes.example("sphere", level=2)
    a, b = geometry.build_plan(7, geom, reorder=False, native=True), geometry.build_plan(7, geom, reorder=False, native=False)
    for name in ("triangles", "corner_ptr", "corner_idx", "lap_rowptr", "lap_col"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in ("hat_grad", "area_tri", "mass_vert", "lap_val"):
        assert np.allclose(getattr(a, name), getattr(b, name), rtol=1e-12, atol=1e-15), name


def test_sampled_step_timers_scale_to_all_iterations():
    """control.SampledStepTimers: per kind of iteration, the first `first` timed iterations count exactly and the others at the
    median of the periodic samples; a slow warm-up iteration is NOT scaled to the whole run; records of one iteration that
    arrive in pieces (time-slab stages) are one sample."""
    from dots_socp_amd.control import RunningHistory, SampledStepTimers, KKT_LABELS, KKT_SHORT_LABELS

    hist = RunningHistory(max_record_numbers=10, kkt_labels=KKT_LABELS, kkt_short_labels=KKT_SHORT_LABELS, name="t")
    tm = SampledStepTimers(hist, first=2, every=5)
    sampled = []
    for i in range(20):
        kind = "read-back" if i % 4 == 0 else "quiet"
        if tm.begin(kind):
            sampled.append((i, kind))
            warm = 40.0 if i < 2 else 0.0                  # the run's first iterations are slow (cold kernels)
            tm.add(kind, "a", (2.0 if kind == "quiet" else 5.0) + warm)
            tm.add(kind, "b", 0.25, 0)                     # two stage records ...
            tm.add(kind, "b", 0.75)                        # ... of one iteration
    tm.publish()
    assert [i for i, _ in sampled] == [0, 1, 2, 4, 6, 13, 16, 19]        # first two of each kind, then every fifth of its kind
    # quiet: 15 iterations = 42 + 2 exactly + 13 x median(2, 2); read-back: 5 = 45 + 5 exactly + 3 x median(5, 5)
    assert hist.steps_time["a"] == pytest.approx(42.0 + 2.0 + 13 * 2.0 + 45.0 + 5.0 + 3 * 5.0)
    assert hist.steps_time["b"] == pytest.approx(20.0)
    assert "20 iterations" in hist.steps_time_note and "8 timed" in hist.steps_time_note
    # before the first periodic sample the latest timed iteration stands in for the rest (not the warm-up mean)
    early = SampledStepTimers(hist, first=2, every=50)
    for i in range(10):
        if early.begin("quiet"):
            early.add("quiet", "a", 40.0 if i == 0 else 2.0)
    early.publish()
    assert hist.steps_time["a"] == pytest.approx(40.0 + 2.0 + 8 * 2.0)
    every = SampledStepTimers(hist, first=0, every=1)
    for _ in range(3):
        assert every.begin("quiet")
        every.add("quiet", "a", 1.5)
    every.publish()
    assert hist.steps_time["a"] == pytest.approx(4.5) and hist.steps_time_note is None


def test_bench_launches_its_own_ranks(monkeypatch, capsys):
    """``python bench.py --gpus N`` without a launcher starts N ranks under torch.distributed.run BEFORE anything touches the GPU,
    lets exactly rank 0's JSON line through on stdout (gloo announces its connections there too) and returns the ranks' exit code
    (VERDICT r2 item 1)."""
    import importlib.util
    import subprocess
    import types

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_run(cmd, env=None, stdout=None, text=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        out = '[Gloo] Rank 0 is connected to 1 peer ranks.\n{"metric": "ALM iterations/s", "value": 1.0, "n_gpus": 2}\n'
        return types.SimpleNamespace(returncode=seen.get("rc", 0), stdout=out if seen.get("json", True) else "[Gloo] noise\n")

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = bench.parse()
    assert bench.launch_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=2" in cmd
    # (the launcher picks the rendezvous port itself, on the loopback address: no bind-and-close race, no host name to resolve)
    assert "--standalone" in cmd and cmd[cmd.index("--local-addr") + 1] == "127.0.0.1" and "--master-port" not in cmd
    assert cmd[-6:] == ["--gpus", "2", "--steps", "20", "--warmup", "5"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert out.out.strip() == '{"metric": "ALM iterations/s", "value": 1.0, "n_gpus": 2}' and "Gloo" in out.err
    # the ranks' failure is the script's failure; no JSON line from the ranks is a failure too
    seen["rc"] = 3
    assert bench.launch_ranks(args) == 3
    seen["rc"], seen["json"] = 0, False
    assert bench.launch_ranks(args) == 1
    # main() takes that path only when no launcher set WORLD_SIZE
    seen["json"] = True
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """``bench.py --dump-outputs DIR``: every state array but z_mid as float64 DIR/<name>.npy, as the solver hands it out
    (recovered); a rank other than 0 takes part in the (collective) downloads and writes nothing; above the size cap every array
    keeps the same fraction of its entries, at the same positions in every run."""
    import importlib.util
    import types

    from dots_socp_amd.device import STATE_NAMES

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class FakeSolver:
        def __init__(self, shape):
            self.dev = types.SimpleNamespace(full_shape=lambda name: shape)
            self.shape, self.downloads = shape, []

        def _download(self, name):
            self.downloads.append(name)
            return np.arange(np.prod(self.shape), dtype=np.float64).reshape(self.shape) + STATE_NAMES.index(name)

        def recovered(self, name, arr):
            return 2.0 * arr

    names = [n for n in STATE_NAMES if n != "z_mid"]
    bench.dump_outputs(FakeSolver((3, 4)), str(tmp_path / "whole"), True)
    assert sorted(os.listdir(tmp_path / "whole")) == sorted(f"{n}.npy" for n in names)
    for n in names:
        got = np.load(tmp_path / "whole" / f"{n}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, 2.0 * (np.arange(12.0).reshape(3, 4) + STATE_NAMES.index(n)))
    other = FakeSolver((3, 4))
    bench.dump_outputs(other, str(tmp_path / "other_rank"), False)
    assert other.downloads == names and not (tmp_path / "other_rank").exists()

    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 100 * len(names))       # room for 100 of the 1000 entries of each array
    for d in ("first", "second"):
        bench.dump_outputs(FakeSolver((10, 100)), str(tmp_path / d), True)
    written = 0
    for n in names:
        a, b = np.load(tmp_path / "first" / f"{n}.npy"), np.load(tmp_path / "second" / f"{n}.npy")
        assert a.dtype == np.float64 and a.shape == (100,) and np.array_equal(a, b)
        assert np.all(np.diff(a) > 0) and np.all((a - 2.0 * STATE_NAMES.index(n)) % 2.0 == 0)       # distinct entries, in order
        written += a.nbytes
    assert written <= bench.DUMP_BYTES


def test_native_assembly_matches_the_numpy_reference():
    """dots_assemble (host code of the library) against the numpy functions of geometry.py, which the oracle tests pin to the
    reference's assembly (surface_pre_computations_socp.py:11-132): areas, hat gradients, masses and corner lists identical,
    K equal to rounding (its entries are summed in a different order) on the same sorted pattern."""
    from dots_socp_amd import geometry, meshes

    for v, t in (meshes.icosphere(3), meshes.torus(40, 24), meshes.plane(12)[:2], meshes.torus_knot_tube(nu=96, nv=8)):
        t = np.asarray(t)
        area, hat, mass, cptr, cidx, K = geometry.assemble_native(v, t)
        area0, hat0 = geometry.hat_gradients(v, t)
        assert np.allclose(area, area0, rtol=1e-15, atol=0) and np.allclose(hat, hat0, rtol=1e-13, atol=1e-15)
        mass0 = np.zeros(v.shape[0])
        for k in range(3):
            np.add.at(mass0, t[:, k], area0)
        assert np.allclose(mass, mass0 / 3.0, rtol=1e-15, atol=0)
        cptr0, cidx0 = geometry.corner_lists(v.shape[0], t)
        assert np.array_equal(cptr, cptr0) and np.array_equal(cidx, cidx0)
        K0 = geometry.stiffness_matrix(v.shape[0], t, area0, hat0)
        assert K.has_sorted_indices and K.shape == K0.shape
        d = abs(K - K0)
        assert d.max() <= 1e-13 * abs(K0).max()
        assert abs(np.asarray(K.sum(axis=1))).max() <= 1e-12 * abs(K0).max()          # rows of the cotangent matrix sum to zero
    with pytest.raises(Exception, match="out of range"):
        geometry.assemble_native(v, np.array([[0, 1, v.shape[0]]]))
