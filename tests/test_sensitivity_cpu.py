"""CPU tests of the cost gradients (dots_socp_amd/sensitivity.py): the specification of dots_sensitivity against the kinetic energy
written directly, its behaviour under a renumbering, the three identities on the fp64 oracle (K = cost; the potentials are the
derivative in the end masses; -dK/dx at fixed stress is the shape derivative -- and holding the densities fixed is not), the
refusals before the library is loaded, and the C ABI.  The device side is test_hip_sensitivity.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import flow_checks as fc
import sensitivity_checks as sc
from conftest import ROOT, load_oracle
from dots_socp_amd import _lib, meshes, sensitivity


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("name", sc.MESHES)
def test_stress_gives_the_kinetic_energy_written_directly(name):
    """kinetic_energy(stress_host(...)) is K as a plain sum over t, f and the corners: to 1e-13 relative (two orders of summation of
    at most 300 * 192 * 3 positive terms in fp64)."""
    v, t = fc.mesh_of(name)
    mass = sc.vertex_masses(v, t)
    for T in (1, 2, 7, 31):
        mu, phi = sc.random_state(name, T)
        stress = sensitivity.stress_host(mu, phi, t, mass)
        assert stress.shape == (t.shape[0], 3, 6) and np.all(stress[:, :, (0, 3, 5)] >= 0.0) and np.any(stress[:, :, 1] != 0.0)
        K, direct = sensitivity.kinetic_energy(stress, v, t, T), sc.kinetic_energy_direct(mu, phi, v, t)
        assert direct > 0.0 and sc.relative(K, direct) <= 1e-13, (name, T, K, direct)
        torch_K = float(sensitivity.kinetic_energy_torch(stress, v, t, T))
        assert sc.relative(torch_K, direct) <= 1e-13
        # the recovery factors are one multiplication each, before anything else
        scaled = sensitivity.stress_host(mu, phi, t, mass, sc.FACTOR_MU, sc.FACTOR_PHI)
        assert same(scaled, sensitivity.stress_host(sc.FACTOR_MU * mu, sc.FACTOR_PHI * phi, t, mass))
        assert same(scaled, sensitivity.stress_numpy(mu, phi, t, mass, sc.FACTOR_MU, sc.FACTOR_PHI))      # the vectorised twin: the same bits


@pytest.mark.parametrize("name", ["icosphere1", "torus", "plane4"])
def test_a_renumbering_permutes_the_stress(name):
    v, t = fc.mesh_of(name)
    mass = sc.vertex_masses(v, t)
    mu, phi = sc.random_state(name, 5)
    rng = np.random.default_rng(9)
    pv, pf = rng.permutation(v.shape[0]), rng.permutation(t.shape[0])      # new vertex i = old pv[i], new triangle j = old pf[j]
    inv = np.empty_like(pv)
    inv[pv] = np.arange(pv.size)
    stress = sensitivity.stress_host(mu, phi, t, mass)
    renumbered = sensitivity.stress_host(mu[:, pv], phi[:, pv], inv[t[pf]], mass[pv])
    assert same(renumbered, stress[pf]) and not same(renumbered, stress)      # corners keep their index
    p0, pT = sensitivity.potentials_host(phi, sc.FACTOR_PHI)
    assert same(p0, sc.FACTOR_PHI * phi[0]) and same(pT, sc.FACTOR_PHI * phi[-1])
    g0, g1 = sensitivity.potential_gradients(p0, pT)
    assert abs(g0.mean()) < 1e-15 and abs(g1.mean()) < 1e-15 and np.allclose(g0, -(p0 - p0.mean())) and np.allclose(g1, pT - pT.mean())


# ---------------------------------------------------------------------------- the identities, on the oracle
@pytest.fixture(scope="module")
def plane():
    """Everything the oracle tests look at, solved once: the plane example (n = 8, T = 7, tol 1e-7, no congestion), flat for the
    densities and bent for the shape; central differences of the oracle's cost."""
    oracle = load_oracle()

    def solve(geom):
        sol, hist = oracle.solver_socp(sc.PLANE_T, geom, tol=sc.PLANE_TOL, nit=sc.PLANE_NIT)
        return sol, float(hist.history["Transportation cost"][-1])

    def cost(geom):
        return solve(geom)[1]

    def sens_of(geom, sol):
        p0, pT = sensitivity.potentials_host(sol["phi"])
        return {"phi0": p0, "phiT": pT, "n_time": sc.PLANE_T,
                "stress": sensitivity.stress_host(sol["mu"], sol["phi"], geom["triangles"], geom["area_vertices"] / 3.0)}

    flat, bent = sc.plane_geometry(), sc.plane_geometry(bent=True)
    out = {"flat": flat, "bent": bent}
    sol, out["cost"] = solve(flat)
    out["sens"] = sens_of(flat, sol)
    g0, g1, _ = sensitivity.cost_gradients(out["sens"], flat["vertices"], flat["triangles"])
    for key, grad in (("mu0", g0), ("mu1", g1)):
        d = sc.density_direction(flat[key])
        out[key] = (float(grad @ d), sc.central_difference(cost, flat, sc.EPS_DENSITY, **{key: d}))
    sol_b, _ = solve(bent)
    d = sc.shape_direction(bent["vertices"].shape[0])
    gx = sensitivity.cost_gradients(sens_of(bent, sol_b), bent["vertices"], bent["triangles"])[2]
    out["shape"] = (float(np.sum(gx * d)), sc.central_difference(cost, bent, sc.EPS_SHAPE, vertices=d))
    out["wrong"] = sc.densities_held_fixed(sol_b["mu"], sol_b["phi"], bent["vertices"], bent["triangles"], d)
    return out


def test_kinetic_energy_is_the_transport_cost(plane):
    """Measured here: K = 0.037805393457 against the oracle's cost 0.037805393468, relative 3.0e-10; the bound is the project's parity
    bar."""
    g = plane["flat"]
    assert g["vertices"].shape[0] == 90 and g["triangles"].shape[0] == 144
    K = sensitivity.kinetic_energy(plane["sens"]["stress"], g["vertices"], g["triangles"], sc.PLANE_T)
    print(f"K = {K:.12f}, cost = {plane['cost']:.12f}, relative {sc.relative(K, plane['cost']):.2e}")
    assert sc.relative(K, plane["cost"]) <= sc.BOUND_COST


@pytest.mark.parametrize("key", ["mu0", "mu1"])
def test_potentials_are_the_derivative_in_the_end_masses(plane, key):
    """Central difference with eps = 1e-3 along a mean-free direction of L1 norm 1 on the support of the density.  Measured here:
    relative 2.9e-7 (mu0) and 2.0e-5 (mu1); the bound is ten times the worse one."""
    grad, fd = plane[key]
    print(f"d cost / d {key}: gradient {grad:.9e}, finite difference {fd:.9e}, relative {sc.relative(grad, fd):.2e}")
    assert abs(fd) > 1e-3 and sc.relative(grad, fd) <= sc.BOUND_DENSITY


def test_shape_derivative_holds_the_masses_fixed(plane):
    """-dK/dx at fixed stress against a central difference (eps = 5e-4, truncation-limited) of the cost on the bent sheet, every
    vertex moved.  Measured here: relative 1.2e-4; the bound is ten times that.  With the DENSITIES held fixed instead the derivative
    is off by more than a factor of 10 (measured: 0.027 against -0.00073)."""
    grad, fd = plane["shape"]
    print(f"d cost / d x: gradient {grad:.9e}, finite difference {fd:.9e}, relative {sc.relative(grad, fd):.2e}; densities held fixed: {plane['wrong']:.4e}")
    assert abs(fd) > 1e-4 and sc.relative(grad, fd) <= sc.BOUND_SHAPE
    assert abs(plane["wrong"] - fd) > 10.0 * abs(fd)


# ---------------------------------------------------------------------------- options
@pytest.fixture
def no_library(monkeypatch):
    """Any call into the HIP library fails the test: the refusals must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", refuse)


def test_bad_options_are_refused_before_the_library(no_library):
    from dots_socp_amd import socp

    geom, _ = meshes.example("sphere", level=1)
    check = sensitivity.check_sensitivity
    assert check(None) is None and check(False) is None and check(None, time_slab=(0, 2), congestion=1.0) is None      # the default changes nothing
    assert check(True) == {"potentials": True, "stress": True, "to_device": False} == check({})
    assert check({"stress": False}, congestion=0.1) == {"potentials": True, "stress": False, "to_device": False}      # the potentials are still returned
    for drive in (socp.solver, socp.solver_raw, socp.solver_socp, socp.solver_cascade, socp.solver_socp_cascade, socp.solver_auto_cascade):
        with pytest.raises(ValueError, match="unknown option"):
            drive(15, geom, sensitivity={"stres": True})
        with pytest.raises(ValueError, match="True or False"):
            drive(15, geom, sensitivity={"stress": 1})
        with pytest.raises(ValueError, match="nothing asked for"):
            drive(15, geom, sensitivity={"stress": False, "potentials": False})
        with pytest.raises(ValueError, match="congestion"):
            drive(15, geom, sensitivity=True, congestion=0.05)
        with pytest.raises(ValueError, match="None, True or a dict"):
            drive(15, geom, sensitivity="stress")
    for drive in (socp.solver, socp.solver_raw, socp.solver_cascade):
        with pytest.raises(ValueError, match="time slabs"):
            drive(15, geom, sensitivity=True, time_slab=(0, 2))
    for drive in (socp.solver_mesh_cascade, socp.solver_socp_mesh_cascade, socp.solver_socp_spacetime_cascade):
        with pytest.raises(ValueError, match="congestion"):
            drive(15, [geom, geom], sensitivity=True, congestion=0.05)
    for drive in (socp.solver_many, socp.solver_socp_many):
        with pytest.raises(ValueError, match="congestion"):      # per problem
            drive(15, geom, [{}, {"congestion": 0.05}], sensitivity=True)
        with pytest.raises(ValueError, match="unknown option"):
            drive(15, geom, [{}], sensitivity={"potential": True})


# ---------------------------------------------------------------------------- C ABI
def test_header_exports_and_version_agree_on_the_entry(tmp_path):
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        text = fh.read()
    assert "int dots_sensitivity(dots_ctx *ctx, const dots_sensitivity_desc *desc);" in text
    assert re.search(r"#define\s+DOTS_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7      # an addition: the ABI version stays
    assert "dots_sensitivity" in _lib.EXPORTS
    lib = _lib.load(host_only=True)
    assert hasattr(lib, "dots_sensitivity") and lib.dots_abi_version() == 7
    fields = [n for n, _ in _lib.SensitivityDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(dots_sensitivity_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(dots_sensitivity_desc, {n}));\n' for n in fields) + "return 0;}\n")
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    out = [int(x) for x in os.popen(str(exe)).read().split()]
    assert out == [ctypes.sizeof(_lib.SensitivityDesc)] + [getattr(_lib.SensitivityDesc, n).offset for n in fields]
