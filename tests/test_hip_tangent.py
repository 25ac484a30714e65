"""GPU tests of linearised transport: dots_tangent_velocities, dots_tangent_weights and dots_tangent_gram against their specifications
(tangent.velocities_host, weights_host, gram_host) on random inputs, their refusals, and socp.tangent_embedding / distance_matrix on
the plane experiment against solver_socp_many, the specification and the exact pair solves; what crosses to the host and what is
built."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tangent_checks as tc
from conftest import has_gpu
from dots_socp_amd import _lib, tangent

ss = importlib.import_module("dots_socp_amd.socp.solver_socp")      # (the package exports the function of this name)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


_contexts = {}


@pytest.fixture(scope="module")
def context():
    """One context per mesh of the kernel tests (nothing is solved on them), closed when the module is done."""
    from dots_socp_amd.device import DeviceProblem

    def get(name):
        if name not in _contexts:
            _contexts[name] = DeviceProblem(1, tc.kernel_geometry(name), lap_solver="spacetime_pcg", reorder="nd")
        return _contexts[name]
    yield get
    for dev in _contexts.values():
        dev.close()
    _contexts.clear()


def on_device(dev, a, dtype=np.float64):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=torch.device("cuda", dev.device)).clone()


@pytest.mark.parametrize("n", tc.KERNEL_N)
@pytest.mark.parametrize("name", list(tc.KERNEL_MESHES))
def test_the_kernels_equal_their_specifications(name, n, context):
    from dots_socp_amd import device

    dev = context(name)
    V, F = dev.V, dev.F
    if name == "torus":
        assert not np.array_equal(dev.plan.perm_vert, np.arange(V))      # the context's numbering is not the caller's
    host = device.caller_tables(dev.plan)
    mesh = dev.tangent_mesh()
    assert mesh is dev.tangent_mesh() and all(np.array_equal(mesh[k].cpu().numpy(), host[k]) for k in host)
    assert np.array_equal(host["triangles"], tc.kernel_mesh(name)[1])
    potentials, sigma = tc.kernel_inputs(name, n)
    vel_want = tangent.velocities_host(potentials, host["triangles"], host["hat"])
    w_want = tangent.weights_host(sigma, host["mass"], host["triangles"], host["area"])
    G_want = tangent.gram_host(vel_want, None, w_want)
    assert np.max(np.abs(vel_want)) > 0.1 and np.all(np.diag(G_want) > 0.0)      # kernels that do nothing cannot pass
    phi = [on_device(dev, p) for p in potentials]
    sigma_d = on_device(dev, sigma)
    before = dev.debug_counter(9)
    vel, w = dev.tangent_velocities(phi), dev.tangent_weights(sigma_d)
    assert tuple(vel.shape) == (n, F, 3) and tuple(w.shape) == (F,)
    assert np.array_equal(bits(vel.cpu().numpy()), bits(vel_want)) and np.array_equal(bits(w.cpu().numpy()), bits(w_want))
    G = dev.tangent_gram(vel, None, w)
    assert dev.debug_counter(9) == before and all(dev.tangent_ms[k] > 0.0 for k in ("velocities", "weights", "gram"))      # (no context is involved)
    bound = tc.gram_bound(G_want, vel_want, None, w_want)
    print(name, n, "max |G - host| / bound", float(np.max(np.abs(G - G_want) / bound)), "in ulp", float(np.max(np.abs(G - G_want) / np.spacing(np.abs(G_want)))))
    assert G.shape == (n, n) and np.all(np.abs(G - G_want) <= bound)
    assert np.array_equal(bits(G), bits(G.T))                                    # symmetric bit for bit
    assert np.array_equal(bits(dev.tangent_gram(vel, None, w)), bits(G))         # two calls, the same bits
    assert np.array_equal(bits(dev.tangent_gram(vel, vel.clone(), w)), bits(G))  # B given is B = A
    if n >= 2:      # a block computed alone is that block of the whole: an entry's order of summation depends on F alone
        k = n // 2
        assert np.array_equal(bits(dev.tangent_gram(vel[:k], vel[k:], w)), bits(G[:k, k:]))
        assert np.array_equal(bits(dev.tangent_gram(vel[k:], vel[:1], w)), bits(G[k:, :1]))
    for p, want in zip(phi, potentials):
        assert np.array_equal(bits(p.cpu().numpy()), bits(want))      # the potentials are read only
    if n in (3, 17):      # through a permuted numbering of the caller's own: the fields are permuted, bit for bit
        pv, pf = tc.renumbering(V, F, seed=n)
        _, t2 = tc.renumbered(tc.kernel_mesh(name)[0], host["triangles"].astype(np.int64), pv, pf)
        other = {"triangles": on_device(dev, t2, np.int32), "hat": on_device(dev, host["hat"][pf]), "area": on_device(dev, host["area"][pf]),
                 "mass": on_device(dev, host["mass"][pv])}
        vel2, _ = device.tangent_velocities(other, [on_device(dev, p[pv]) for p in potentials])
        w2, _ = device.tangent_weights(other, on_device(dev, sigma[pv]))
        assert np.array_equal(bits(vel2.cpu().numpy()), bits(vel_want[:, pf])) and np.array_equal(bits(w2.cpu().numpy()), bits(w_want[pf]))
        G2, _ = device.tangent_gram(vel2, None, w2)
        assert np.all(np.abs(G2 - G_want) <= bound)


def test_refusals_launch_nothing(context):
    import torch

    from dots_socp_amd import device

    dev = context("torus")
    V, F = dev.V, dev.F
    lib = dev.lib
    mesh = dev.tangent_mesh()
    potentials, sigma = tc.kernel_inputs("torus", 2)
    phi = [on_device(dev, p) for p in potentials]
    sigma_d = on_device(dev, sigma)
    where = sigma_d.device
    vel = torch.full((2, F, 3), -1.0, dtype=torch.float64, device=where)
    w = torch.full((F,), -1.0, dtype=torch.float64, device=where)
    need = int(lib.dots_tangent_gram_scratch(2, 2, F))
    assert need == 3 * 4
    scratch = torch.zeros(need + 8, dtype=torch.float64, device=where)
    G = np.full((2, 2), np.nan)
    Gp = G.ctypes.data_as(C.POINTER(C.c_double))
    pointers = (C.c_void_p * 2)(phi[0].data_ptr(), phi[1].data_ptr())
    one_null = (C.c_void_p * 2)(phi[0].data_ptr(), None)
    none = C.cast(None, C.POINTER(C.c_void_p))

    def desc(**change):
        d = _lib.TangentDesc()
        d.device, d.n_vertices, d.n_triangles = dev.device, V, F
        d.triangles, d.hat_grad, d.area_tri, d.mass_vert = (mesh[k].data_ptr() for k in ("triangles", "hat", "area", "mass"))
        d.stream = torch.cuda.current_stream(where).cuda_stream
        for k, v in change.items():
            setattr(d, k, v)
        return d

    def velocities(d, n=2, p=pointers, out=None):
        return lib.dots_tangent_velocities(C.byref(d), n, p, vel.data_ptr() if out is None else out)

    def weights(d, s=None, out=None):
        return lib.dots_tangent_weights(C.byref(d), sigma_d.data_ptr() if s is None else s, w.data_ptr() if out is None else out)

    def gram(d, na=2, A=None, nb=2, B=None, ww=None, s=None, out=Gp):
        return lib.dots_tangent_gram(C.byref(d), na, vel.data_ptr() if A is None else A, nb, B, w.data_ptr() if ww is None else ww,
                                     scratch.data_ptr() if s is None else s, out)

    cases = [("velocities: n = 0", lambda: velocities(desc(), n=0)), ("velocities: n < 0", lambda: velocities(desc(), n=-3)),
             ("velocities: no potentials", lambda: velocities(desc(), p=none)), ("velocities: a null potential", lambda: velocities(desc(), p=one_null)),
             ("velocities: V = 0", lambda: velocities(desc(n_vertices=0))), ("velocities: F = 0", lambda: velocities(desc(n_triangles=0))),
             ("velocities: no triangles", lambda: velocities(desc(triangles=None))), ("velocities: no hat", lambda: velocities(desc(hat_grad=None))),
             ("velocities: the output is a potential", lambda: velocities(desc(), out=phi[1].data_ptr() + 8 * (V - 1))),
             ("velocities: the output is the hat table", lambda: velocities(desc(), out=mesh["hat"].data_ptr() + 8)),
             ("weights: no sigma", lambda: lib.dots_tangent_weights(C.byref(desc()), None, w.data_ptr())),
             ("weights: no output", lambda: lib.dots_tangent_weights(C.byref(desc()), sigma_d.data_ptr(), None)),
             ("weights: no areas", lambda: weights(desc(area_tri=None))), ("weights: no masses", lambda: weights(desc(mass_vert=None))),
             ("weights: no triangles", lambda: weights(desc(triangles=None))), ("weights: F < 0", lambda: weights(desc(n_triangles=-1))),
             ("weights: the output is sigma", lambda: weights(desc(), out=sigma_d.data_ptr() - 8 * (F - 1))),
             ("weights: the output is the areas", lambda: weights(desc(), out=mesh["area"].data_ptr())),
             ("gram: na = 0", lambda: gram(desc(), na=0)), ("gram: nb = 0", lambda: gram(desc(), nb=0, B=vel.data_ptr())),
             ("gram: na = 4097", lambda: gram(desc(), na=4097)), ("gram: B = NULL with nb != na", lambda: gram(desc(), nb=1)),
             ("gram: F = 0", lambda: gram(desc(n_triangles=0))),
             ("gram: no A", lambda: lib.dots_tangent_gram(C.byref(desc()), 2, None, 2, None, w.data_ptr(), scratch.data_ptr(), Gp)),
             ("gram: no w", lambda: lib.dots_tangent_gram(C.byref(desc()), 2, vel.data_ptr(), 2, None, None, scratch.data_ptr(), Gp)),
             ("gram: no scratch", lambda: lib.dots_tangent_gram(C.byref(desc()), 2, vel.data_ptr(), 2, None, w.data_ptr(), None, Gp)),
             ("gram: no G", lambda: gram(desc(), out=C.cast(None, C.POINTER(C.c_double)))),
             ("gram: scratch and A overlap", lambda: gram(desc(), s=vel.data_ptr() + 8 * (2 * F * 3 - 1))),
             ("gram: scratch and B overlap", lambda: gram(desc(), B=scratch.data_ptr() + 8 * (need - 1))),
             ("gram: scratch and w overlap", lambda: gram(desc(), s=w.data_ptr() - 8 * (need - 1)))]
    for what, call in cases:
        assert call() == _lib.ERR_ARGUMENT, what
        assert "tangent_" + what.split(":")[0] in lib.dots_last_error().decode(), what
    assert lib.dots_tangent_velocities(None, 2, pointers, vel.data_ptr()) == _lib.ERR_ARGUMENT
    assert lib.dots_tangent_weights(None, sigma_d.data_ptr(), w.data_ptr()) == _lib.ERR_ARGUMENT
    assert lib.dots_tangent_gram(None, 2, vel.data_ptr(), 2, None, w.data_ptr(), scratch.data_ptr(), Gp) == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert float(vel.min()) == float(vel.max()) == -1.0 and float(w.min()) == float(w.max()) == -1.0      # nothing launched
    assert np.all(np.isnan(G)) and float(scratch.abs().sum()) == 0.0
    # the calls as they should be: the scratch is used to its stated length only
    assert velocities(desc()) == 0 and weights(desc()) == 0 and gram(desc()) == 0
    host = device.caller_tables(dev.plan)
    want = tangent.velocities_host(potentials, host["triangles"], host["hat"])
    assert np.array_equal(bits(vel.cpu().numpy()), bits(want)) and np.all(np.isfinite(G))
    assert np.array_equal(scratch[need:].cpu().numpy(), np.zeros(8))
    # the wrappers' own checks
    with pytest.raises(ValueError, match="every potential must be"):
        dev.tangent_velocities([p.to(torch.float32) for p in phi])
    with pytest.raises(ValueError, match="every potential must be"):
        dev.tangent_velocities([p.cpu() for p in phi])
    with pytest.raises(ValueError, match="no potentials"):
        dev.tangent_velocities([])
    with pytest.raises(ValueError, match="sigma must be"):
        dev.tangent_weights(sigma_d[:-1])
    with pytest.raises(ValueError, match="must hold tensors"):
        device.tangent_weights({k: v for k, v in mesh.items() if k != "area"}, sigma_d)
    with pytest.raises(ValueError, match="A must be"):
        dev.tangent_gram(vel[0], None, w)
    with pytest.raises(ValueError, match="B must have shape"):
        dev.tangent_gram(vel, vel[:, :-1].contiguous(), w)
    with pytest.raises(ValueError, match="w must be"):
        dev.tangent_gram(vel, None, w[:-1])


def test_a_time_slab_has_no_tangent_calls():
    from dots_socp_amd.device import DeviceProblem

    with DeviceProblem(3, tc.kernel_geometry("plane4"), lap_solver="modal_pcg", reorder="nd", time_slab=(0, 2)) as dev:
        with pytest.raises(ValueError, match="time slabs"):
            dev.tangent_mesh()
        with pytest.raises(ValueError, match="time slabs"):
            dev.tangent_weights(on_device(dev, np.ones(dev.V)))


# ---- the drivers on the plane experiment ---------------------------------------------------------------------------------------------
class Recorded:
    """The device calls of ``tangent_embedding`` with a record of what they received, of what the contexts had copied to the host and
    of what had been built"""

    def __init__(self, monkeypatch):
        from dots_socp_amd.device import DeviceProblem

        self.made, self.plans, self.factors, self.calls = [], [], [], {}
        rec = self

        def state():
            return {"d2h": sum(d.debug_counter(9) for d in rec.made), "made": len(rec.made), "plans": len(rec.plans), "factors": len(rec.factors)}

        inner_v, inner_g = DeviceProblem.tangent_velocities, DeviceProblem.tangent_gram

        def velocities(dev, potentials):
            rec.calls["before"] = state()
            rec.calls["potentials"] = [p.cpu().numpy() for p in potentials]
            rec.calls["plan"] = dev.plan
            return inner_v(dev, potentials)

        def gram(dev, A, B, w):
            G = inner_g(dev, A, B, w)
            rec.calls["after"] = state()
            return G

        class Counted(ss.DeviceProblem):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                rec.made.append(self)

            def setup_frontal(self, *a, **kw):
                rec.factors.append(1)
                return super().setup_frontal(*a, **kw)

        import dots_socp_amd.geometry as geo

        build_plan = geo.build_plan

        def counted_plan(*a, **kw):
            rec.plans.append(1)
            return build_plan(*a, **kw)

        monkeypatch.setattr(DeviceProblem, "tangent_velocities", velocities)
        monkeypatch.setattr(DeviceProblem, "tangent_gram", gram)
        monkeypatch.setattr(ss, "DeviceProblem", Counted)
        monkeypatch.setattr(geo, "build_plan", counted_plan)


def test_the_embedding_equals_the_batch_solves_and_the_specification(monkeypatch):
    from dots_socp_amd import device, socp

    geom, sigma, measures, moves = tc.plane_case()
    N, F = len(measures), geom["triangles"].shape[0]
    request = {"potentials": True, "stress": False}
    want = socp.solver_socp_many(tc.PLANE_T, geom, [{"mu0": sigma, "mu1": m, "tol": tc.PLANE_TOL_DEVICE} for m in measures], outputs=(),
                                 sensitivity=request)
    rec = Recorded(monkeypatch)
    r = socp.tangent_embedding(tc.PLANE_T, geom, sigma, measures, velocities=True, tol=tc.PLANE_TOL_DEVICE)
    # costs and potentials: the batch driver's bits
    assert np.array_equal(bits(r["costs"]), bits([hist.history["Transportation cost"][-1] for _, hist in want]))
    assert list(r["iterations"]) == [int(hist.kkt_iteration[-1]) + 1 for _, hist in want]
    for i in range(N):
        assert np.array_equal(bits(rec.calls["potentials"][i]), bits(want[i][0]["sensitivity"]["phi0"])), i
    # velocities, weights and G: the specification on those potentials with the tables the contexts hold
    host = device.caller_tables(rec.calls["plan"])
    vel = tangent.velocities_host(np.stack(rec.calls["potentials"]), host["triangles"], host["hat"])
    w = tangent.weights_host(sigma, host["mass"], host["triangles"], host["area"])
    G = tangent.gram_host(vel, None, w)
    assert np.array_equal(bits(r["velocities"]), bits(vel)) and np.array_equal(bits(r["weights"]), bits(w))
    assert np.all(np.abs(r["gram"] - G) <= tc.gram_bound(G, vel, None, w)) and np.array_equal(bits(r["gram"]), bits(r["gram"].T))
    assert np.array_equal(r["squared_distances"], tangent.squared_distances(r["gram"]))
    # after the solves nothing of a context crosses to the host, and nothing is built after the first admission
    assert rec.calls["after"]["d2h"] == rec.calls["before"]["d2h"]
    assert r["solver_stats"]["bytes_to_host"] == 8 * N * N + 8 * F + 24 * N * F      # G; the weights and the velocities that were asked for
    assert (rec.calls["after"]["made"], rec.calls["after"]["plans"], rec.calls["after"]["factors"]) == (N, 1, 1)
    # the linearisation, at 1.5 times the bounds of the oracle's run
    pair_costs = {}
    pairs = socp.solver_socp_many(tc.PLANE_T, geom, [{"mu0": measures[i], "mu1": measures[j], "tol": tc.PLANE_TOL_DEVICE} for i, j in tc.PLANE_PAIRS],
                                  outputs=())
    for (i, j), (_, hist) in zip(tc.PLANE_PAIRS, pairs):
        pair_costs[(i, j)] = float(hist.history["Transportation cost"][-1])
    own, pair_errors, mean = tc.plane_figures(r["gram"], r["costs"], r["velocities"], r["weights"], moves, pair_costs)
    print("G_ii / (2 cost_i)", [float(r["gram"][i, i] / (2.0 * r["costs"][i])) for i in range(N)], "pairs", pair_errors, "mean velocity", mean,
          "tangent_ms", r["solver_stats"]["tangent_ms"])
    assert own <= tc.DEVICE_MARGIN * tc.BOUND_SELF and max(pair_errors) <= tc.DEVICE_MARGIN * tc.BOUND_PAIR and mean <= tc.DEVICE_MARGIN * tc.BOUND_MEAN


def test_more_measures_than_slots_and_results_on_the_device(monkeypatch):
    """Four measures on two contexts: a slot that finishes takes the next problem by a restart; the same bits, nothing more built.  With
    ``to_device`` only G crosses."""
    import torch

    from dots_socp_amd import socp

    geom, sigma, measures, _ = tc.plane_case()
    N = len(measures)
    whole = socp.tangent_embedding(tc.PLANE_T, geom, sigma, measures, velocities=True, tol=tc.PLANE_TOL_DEVICE)
    rec = Recorded(monkeypatch)
    r = socp.tangent_embedding(tc.PLANE_T, geom, sigma, measures, velocities=True, to_device=True, max_batch=2, tol=tc.PLANE_TOL_DEVICE)
    assert (rec.calls["after"]["made"], rec.calls["after"]["plans"], rec.calls["after"]["factors"]) == (2, 1, 1)
    assert rec.calls["after"]["d2h"] == rec.calls["before"]["d2h"] and r["solver_stats"]["bytes_to_host"] == 8 * N * N
    assert isinstance(r["velocities"], torch.Tensor) and r["velocities"].is_cuda and r["weights"].is_cuda
    assert np.array_equal(bits(r["gram"]), bits(whole["gram"])) and np.array_equal(bits(r["costs"]), bits(whole["costs"]))
    assert np.array_equal(bits(r["velocities"].cpu().numpy()), bits(whole["velocities"]))
    assert socp.tangent_embedding(tc.PLANE_T, geom, sigma, measures[:1], tol=tc.PLANE_TOL_DEVICE)["velocities"] is None


def test_the_distance_matrix_against_the_exact_pairs():
    """All six pairs of the plane's four Gaussians: the linearisation at the set-up's reference within 1.5 times the oracle run's pair
    bound of the exact solves.  From the default reference, the mean of the four -- not a Gaussian, so the maps are no translations --
    the figure is printed, not bounded."""
    from dots_socp_amd import socp

    geom, sigma, measures, _ = tc.plane_case()
    exact = socp.distance_matrix(tc.PLANE_T, geom, measures, method="pairs", tol=tc.PLANE_TOL_DEVICE)
    linear = socp.distance_matrix(tc.PLANE_T, geom, measures, reference=sigma, tol=tc.PLANE_TOL_DEVICE)
    from_mean = socp.distance_matrix(tc.PLANE_T, geom, measures, tol=tc.PLANE_TOL_DEVICE)
    off = ~np.eye(len(measures), dtype=bool)
    error = np.abs(linear - exact)[off] / exact[off]
    print("relative difference from the exact pairs: reference", float(error.max()), "mean of the measures", float((np.abs(from_mean - exact)[off] / exact[off]).max()))
    assert exact.shape == (4, 4) and np.array_equal(exact, exact.T) and np.all(np.diag(exact) == 0.0) and np.all(exact[off] > 0.0)
    assert np.array_equal(linear, linear.T) and np.all(np.diag(linear) == 0.0)
    assert error.max() <= tc.DEVICE_MARGIN * tc.BOUND_PAIR
