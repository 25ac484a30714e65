"""What the tests of the push-forward (dots_flow_push) share, on top of flow_checks.py (TEST INFRASTRUCTURE, plain numpy): what the
particles carry, the specification with the exponents of push_scales, and bitwise comparison."""
import numpy as np

import flow_checks as fc
from dots_socp_amd import flow

ATTRIBUTE_COUNTS = (0, 1, 4)
LAYERS = ("end", "all")


def same(a, b):
    """== on every element, and on the bits of the floating-point ones (a NaN or a signed zero would differ)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))
    return np.array_equal(a, b)


def carried(n_particles, n_attributes, seed=0):
    """``(mass (P,), attributes (A, P) or None)``: masses in (0.1, 1.1), attributes of both signs and several magnitudes."""
    rng = np.random.default_rng(3000 + seed)
    mass = 0.1 + rng.random(n_particles)
    if n_attributes == 0:
        return mass, None
    attributes = rng.standard_normal((n_attributes, n_particles)) * (10.0 ** np.arange(n_attributes))[:, None]
    assert np.any(attributes < 0.0) and np.any(attributes > 0.0)
    return mass, attributes


def specification(host, triangles, n_vertices, mass, attributes, layers, exponents=None):
    """``push_forward_host`` on a host result with its trajectory, with the exponents of ``push_scales`` for the starts (layer 0)."""
    if exponents is None:
        exponents = flow.push_scales(mass, attributes, host["weights_at"][0])
    return flow.push_forward_host(host, triangles, n_vertices, mass, attributes, exponents, layers)


def assert_pushed_equals(got_mass, got_attr, got_dropped, want, what=""):
    assert same(got_mass, want["mass"]), (what, "mass")
    if want["attributes"] is None:
        assert got_attr is None, (what, "attributes")
    else:
        assert same(got_attr, want["attributes"]), (what, "attributes")
    assert got_dropped == want["dropped"], (what, "dropped", got_dropped, want["dropped"])


def small_trajectory(name="icosphere1", count=200):
    """A host trajectory of a case of flow_checks (random state, vertex and interior starts): ``(host, triangles, V)``."""
    from dots_socp_amd.geometry import hat_gradients

    v, t = fc.mesh_of(name)
    mu, E = fc.random_state(name)
    tri, w = fc.particles(name, count)
    _, hat = hat_gradients(v, t)
    host = flow.flow_map_host(mu, E, t, hat, flow.triangle_neighbours(t), tri, w, fc.FLOOR, max_crossings=fc.CASES[name][4], trajectory=True)
    return host, t, v.shape[0]
