"""CPU tests of the cascade in space and time at once: the specification (cascade.carry_spacetime) against the composition of the two
existing specifications, its argument checks and exactness properties, the default levels and the level checks of the driver, the
driver's argument errors before any device call, and the entry point in the header and the library."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from carry_checks import STATE
from conftest import ROOT
from dots_socp_amd import _lib, cascade, meshes


def on_sphere(p):
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def shapes(n, V, F):
    return {"phi": (n + 1, V), "B": (n + 1, F, 3), "E": (n + 1, F, 3), "z_mid": (n, 2, 3, F, 3), "beta_mid": (n, 2, 3, F, 3),
            **{k: (n, V) for k in ("A", "lambda_c", "z_fst", "z_end", "mu", "beta_fst", "beta_end")}}


def maps(kind):
    """(V, F of the source, V, F of the destination, the keyword of the map): plane(4) to its subdivision, or to plane(7)"""
    v, t = meshes.plane(4)
    if kind == "nested":
        vf, tf, parents = meshes.subdivide(v, t)
        return v.shape[0], t.shape[0], vf.shape[0], tf.shape[0], {"parents": parents}
    vf, tf = meshes.plane(7)
    transfer = cascade.mesh_transfer({"vertices": v, "triangles": t}, {"vertices": vf, "triangles": tf})
    return v.shape[0], t.shape[0], vf.shape[0], tf.shape[0], {"transfer": transfer}


@pytest.mark.parametrize("kind", ["nested", "located"])
@pytest.mark.parametrize("grids", [(1, 3), (3, 7), (5, 7), (6, 13), (7, 3)])
def test_specification_is_space_then_time(kind, grids):
    n_src, n_dst = grids
    Vs, Fs, Vd, Fd, how = maps(kind)
    src, dst = shapes(n_src, Vs, Fs), shapes(n_dst, Vd, Fd)
    rng = np.random.default_rng(11)
    sol = {k: rng.standard_normal(src[k]) for k in STATE}
    in_space = cascade.prolong_space_solution(sol, how["parents"]) if kind == "nested" else cascade.transfer_space_solution(sol, how["transfer"])
    want = cascade.prolong_solution(in_space, n_src, n_dst)
    sol["checkpoints"] = None
    got = cascade.carry_spacetime_solution(sol, n_src, n_dst, **how)
    assert set(got) == set(STATE)
    for k in STATE:
        one = cascade.carry_spacetime(sol[k], k, n_src, n_dst, **how)
        assert got[k].shape == dst[k] and got[k].dtype == np.float64, k
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k
        assert np.array_equal(one.view(np.int64), want[k].view(np.int64)), k


def test_specification_checks_its_arguments():
    Vs, Fs, _, _, nested = maps("nested")
    located = maps("located")[4]
    x = np.zeros((3, Vs))
    with pytest.raises(ValueError, match="prolong_space"):
        cascade.carry_spacetime(x, "mu", 3, 3, **nested)                        # equal grids: the carriers in space
    with pytest.raises(ValueError):
        cascade.carry_spacetime(x, "mu", 3, 3, **located)
    with pytest.raises(ValueError, match="exactly one"):
        cascade.carry_spacetime(x, "mu", 3, 7, **nested, **located)             # both maps
    with pytest.raises(ValueError, match="exactly one"):
        cascade.carry_spacetime(x, "mu", 3, 7)                                  # neither
    for bad in (dict(nested, **located), {}):
        with pytest.raises(ValueError, match="exactly one"):
            cascade.carry_spacetime_solution({"mu": x}, 3, 7, **bad)
    with pytest.raises(ValueError):
        cascade.carry_spacetime_solution({"mu": x}, 7, 7, **nested)
    with pytest.raises(ValueError):
        cascade.carry_spacetime(x, "rho", 3, 7, **nested)
    with pytest.raises(ValueError):
        cascade.carry_spacetime(np.zeros((4, Vs)), "mu", 3, 7, **nested)        # not the source's time grid


@pytest.mark.parametrize("kind", ["nested", "located"])
def test_constants_are_reproduced_exactly(kind):
    """Nested: copies and (c + c) * 0.5 in space; in time (1 - w) * c + w * c, which for c a power of two is c * fl(fl(1 - w) + w) = c for
    every w in [0, 1] (w >= 1/2: 1 - w is exact; below, it is off by at most 2^-54, which the sum rounds away).  Located: the vertex
    weights sum to 1 to rounding only, so there the constant 0 is what is exact; the triangle and corner arrays are copied in space."""
    Vs, Fs, Vd, Fd, how = maps(kind)
    for n_src, n_dst in ((3, 7), (7, 15), (7, 3)):
        src, dst = shapes(n_src, Vs, Fs), shapes(n_dst, Vd, Fd)
        for k in STATE:
            copied = kind == "nested" or k not in cascade.VERTEX_ARRAYS
            for c in ((1.0, -0.25, 0.0) if copied else (0.0,)):
                out = cascade.carry_spacetime(np.full(src[k], c), k, n_src, n_dst, **how)
                assert out.shape == dst[k] and np.array_equal(out, np.full(dst[k], c)), (k, c)


@pytest.mark.parametrize("kind", ["nested", "located"])
def test_linear_in_time_constant_in_space_on_node_arrays(kind):
    """a(t) = 0.25 + 1.5 t on the nodes, |a| <= 1.75.  The bound: at most eight roundings of values <= 1.75 on the way (three products and
    two sums in space -- the located weights sum to 1 to rounding only --, two products and a sum in time), one ulp each, plus the
    rounding of w itself (a quotient of rounded grid points, ~2 ulp) times the slope across one source interval (<= 1.5): 16 ulp of
    1.75 covers them."""
    Vs, Fs, Vd, Fd, how = maps(kind)
    lin = lambda n: 0.25 + 1.5 * np.arange(n + 1) / n      # noqa: E731
    for n_src, n_dst in ((3, 7), (5, 7), (6, 13), (15, 4)):
        src, dst = shapes(n_src, Vs, Fs), shapes(n_dst, Vd, Fd)
        for k in cascade.NODE_ARRAYS:
            x = np.broadcast_to(lin(n_src).reshape((-1,) + (1,) * (len(src[k]) - 1)), src[k])
            out = cascade.carry_spacetime(x, k, n_src, n_dst, **how)
            want = np.broadcast_to(lin(n_dst).reshape((-1,) + (1,) * (len(dst[k]) - 1)), dst[k])
            assert np.max(np.abs(out - want)) <= 16 * np.finfo(np.float64).eps * 1.75, (k, n_src, n_dst)


def test_default_levels():
    assert cascade.default_spacetime_levels(127, 3) == [31, 63, 127]
    assert cascade.default_spacetime_levels(31, 3) == [15, 15, 31]
    assert cascade.default_spacetime_levels(20, 2) == [20, 20]
    assert cascade.default_spacetime_levels(1023, 2) == [511, 1023]
    assert cascade.check_spacetime_levels(None, 127, 3) == [31, 63, 127]
    assert cascade.check_spacetime_levels([7, 7, 15], 15, 3) == [7, 7, 15]


def test_levels_are_checked():
    for bad in ([7, 15], [3, 7, 15, 15], [15, 7, 15], [3, 7, 31], [0, 7, 15], [3.5, 7, 15], "abc", 7):
        with pytest.raises(ValueError):
            cascade.check_spacetime_levels(bad, 15, 3)


class _Finalised:
    """What the argument checks of AlmSolver read of ``init_from``, without a device"""
    finalized = True

    def __init__(self, n_time):
        self.n_time = n_time


def sphere_levels(n):
    geom, _ = meshes.make_geometry(*meshes.icosphere(1))
    geom["mu0"] = geom["mu1"] = np.full(42, 1.0 / 42)
    return meshes.refine_levels(geom, n, project=on_sphere)


def test_argument_errors_before_any_device_call(monkeypatch):
    from dots_socp_amd import device
    from dots_socp_amd.socp import solver_raw_spacetime_cascade, solver_socp_spacetime_cascade, solver_spacetime_cascade
    from dots_socp_amd.socp.solver_socp import AlmSolver

    def no_device(*args, **kwargs):
        raise AssertionError("a device context was created before the arguments were checked")

    monkeypatch.setattr(device.DeviceProblem, "__init__", no_device)
    levels = sphere_levels(3)
    parents = levels[1]["parents"]
    with pytest.raises(ValueError, match="time grid"):
        AlmSolver(15, levels[1], init_from=_Finalised(7), init_parents=parents)       # without init_regrid: as before
    with pytest.raises(ValueError, match="time grid"):
        AlmSolver(15, levels[1], init_from=_Finalised(7), init_parents=parents, init_regrid=False)
    with pytest.raises(ValueError, match="init_regrid"):
        AlmSolver(15, levels[1], init_from=_Finalised(7), init_regrid=True)           # no map in space
    with pytest.raises(ValueError, match="init_from"):
        AlmSolver(15, levels[1], init_parents=parents, init_regrid=True)
    call = solver_socp_spacetime_cascade
    with pytest.raises(ValueError, match="two geometries"):
        call(7, [levels[1]])
    with pytest.raises(ValueError):
        solver_raw_spacetime_cascade(7, [])
    with pytest.raises(ValueError):
        solver_spacetime_cascade(7, [])
    with pytest.raises(ValueError, match="parents"):
        call(7, [levels[0], {k: v for k, v in levels[1].items() if k != "parents"}, levels[2]])
    with pytest.raises(ValueError, match="one n_time per geometry"):
        call(15, levels, levels=[7, 15])                                              # wrong length
    with pytest.raises(ValueError, match="decrease"):
        call(15, levels, levels=[15, 7, 15])
    with pytest.raises(ValueError, match="last level"):
        call(15, levels, levels=[3, 7, 31])
    with pytest.raises(ValueError):
        call(15, levels, levels=[0, 7, 15])
    with pytest.raises(ValueError):
        call(300, levels, levels=[15, 299, 300], lap_solver="modal_pcg")               # a level the Laplacian solver cannot take
    with pytest.raises(ValueError):
        call(2047, levels, levels=[15, 31, 2047])
    with pytest.raises(ValueError):
        call(15, levels, lap_solver="no_such_solver")
    for bad in (dict(init_from=None), dict(time_slab=(0, 2)), dict(init_parents=parents), dict(level_tol=-1.0), dict(no_such_option=1), dict(nit=0)):
        with pytest.raises(ValueError):
            call(15, levels, **bad)
    # the existing drivers keep their refusals
    from dots_socp_amd.socp import solver_socp_mesh_cascade

    with pytest.raises(ValueError, match="levels"):
        solver_socp_mesh_cascade(7, levels, levels=[3, 7, 7])


TIME_RECORD = ("n_time", "tol", "iterations", "running_time", "setup_seconds", "prolong_ms", "cost", "kkt_max")
MESH_RECORD = ("n_vertices", "n_triangles", "tol", "iterations", "running_time", "setup_seconds", "prolong_ms", "prolong_bytes", "cost", "kkt_max",
               "device_bytes", "transfer", "max_distance")
SPACETIME_RECORD = ("n_time", "n_vertices", "n_triangles", "tol", "iterations", "running_time", "setup_seconds", "prolong_ms", "prolong_bytes", "cost",
                    "kkt_max", "device_bytes", "transfer", "max_distance")
PLUG_IN_NAMES = {"solver_raw": "dot_solver_socp", "solver": "dot_solver_socp_center",
                 "solver_raw_cascade": "dot_solver_socp_cascade", "solver_cascade": "dot_solver_socp_cascade_center",
                 "solver_raw_mesh_cascade": "dot_solver_socp_mesh_cascade", "solver_mesh_cascade": "dot_solver_socp_mesh_cascade_center",
                 "solver_raw_spacetime_cascade": "dot_solver_socp_spacetime_cascade",
                 "solver_spacetime_cascade": "dot_solver_socp_spacetime_cascade_center",
                 "solver_raw_auto_cascade": "dot_solver_socp_auto_cascade", "solver_auto_cascade": "dot_solver_socp_auto_cascade_center"}


class _Level:
    """What a cascade driver touches of an AlmSolver, without a device: a level that stops after one iteration."""
    open_levels = 0

    def __init__(self, n_time, geometry, tol=1e-4, init_from=None, release_init_from=False, **kw):
        self.n_time, self.tol, self.counter_main = n_time, tol, 0
        self.prolong_ms = None if init_from is None else 0.25
        self.dev = types.SimpleNamespace(V=np.asarray(geometry["vertices"]).shape[0], F=np.asarray(geometry["triangles"]).shape[0], sync=lambda: None)
        if init_from is not None:
            assert release_init_from
            init_from.close()
        _Level.open_levels += 1

    def iterate(self):
        return True

    def finalize(self, **kw):
        hist = types.SimpleNamespace(running_time=0.5, history={"Transportation cost": [2.0]}, kkt_errors=np.full((1, 7), 1e-5),
                                     solver_stats={"device_bytes": 1024})
        return {}, hist

    def close(self):
        _Level.open_levels -= 1


def test_level_records_and_plug_in_names(monkeypatch):
    """Every level's record of the three cascade drivers has exactly the driver's fields, in its order; one level is open at a time and
    none is left open; the ten plug-ins keep the names the reference's runner prints."""
    import importlib

    from dots_socp_amd import socp

    module = importlib.import_module("dots_socp_amd.socp.solver_socp")
    monkeypatch.setattr(module, "AlmSolver", _Level)
    levels = sphere_levels(3)
    runs = [("cascade", TIME_RECORD, 2, lambda: module.solver_socp_cascade(31, levels[0], levels=[15, 31])),
            ("mesh_cascade", MESH_RECORD, 3, lambda: module.solver_socp_mesh_cascade(7, levels)),
            ("spacetime_cascade", SPACETIME_RECORD, 3, lambda: module.solver_socp_spacetime_cascade(15, levels, levels=[7, 7, 15]))]
    for key, fields, n, run in runs:
        _, hist = run()
        stats = hist.solver_stats[key]
        assert tuple(stats) == ("levels", "total_seconds") and len(stats["levels"]) == n
        for i, rec in enumerate(stats["levels"]):
            assert tuple(rec) == fields, (key, i, tuple(rec))
            assert (rec["prolong_ms"] is None) == (i == 0)
        assert _Level.open_levels == 0
    for name, printed in PLUG_IN_NAMES.items():
        assert getattr(socp, name).__name__ == printed


def test_header_and_library_have_the_entry_point(tmp_path):
    text = open(os.path.join(ROOT, "include", "dots_socp_hip.h")).read()
    assert "int dots_carry_spacetime(dots_ctx *dst, dots_ctx *src, const dots_carry_spacetime_desc *desc);" in text
    assert "dots_carry_spacetime" in _lib.EXPORTS
    lib = _lib.load(host_only=True)
    assert hasattr(lib, "dots_carry_spacetime")
    assert _lib.ABI_VERSION == 7      # an addition: the ABI version stays
    # the library exports what the header declares and nothing else
    import re

    declared = sorted(set(re.findall(r"^[A-Za-z_][\w \*]*?\b(dots_\w+)\s*\(", text, flags=re.M)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert "dots_carry_spacetime" in exported and set(exported) <= set(declared), sorted(set(exported) - set(declared))
    # the ctypes mirror of the descriptor has the header's layout
    fields = ("node_j", "vsrc", "vw", "fsrc", "csrc", "n_vertices", "n_triangles", "factor", "ms")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
                   'int main(void){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(dots_carry_spacetime_desc)'
                   + "".join(f", offsetof(dots_carry_spacetime_desc, {f})" for f in fields) + "); return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.CarrySpacetimeDesc
    assert out == [C.sizeof(D)] + [getattr(D, f).offset for f in fields]
