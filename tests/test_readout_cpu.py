"""The device read-out (dots_readout) without a GPU: its declaration and binding, the numpy specification against the conversion
the plug-ins did on the host, the layer-sum checks, and the resources of the two kernels in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dots_socp_hip.h")


def test_readout_is_declared_and_bound():
    from dots_socp_amd import _lib

    text = open(HEADER).read()
    assert re.search(r"\bint dots_readout\(dots_ctx \*ctx, const dots_readout_desc \*desc\);", text)
    assert "dots_readout" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 7
    assert re.search(r"#define DOTS_ABI_VERSION 7\b", text)


def test_readout_desc_matches_the_header(tmp_path):
    """Compile a probe with gcc against the header and compare size and offsets with the ctypes mirror."""
    from dots_socp_amd import _lib

    fields = [name for name, _ in _lib.ReadoutDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
        'int main(void){printf("%zu", sizeof(dots_readout_desc));\n'
        + "".join(f'printf(" %zu", offsetof(dots_readout_desc, {f}));\n' for f in fields)
        + "return 0;}\n"
    )
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    out = [int(x) for x in os.popen(str(exe)).read().split()]
    want = [ctypes.sizeof(_lib.ReadoutDesc)] + [getattr(_lib.ReadoutDesc, f).offset for f in fields]
    assert out == want
    assert fields == ["factor", "w_vertex", "w_triangle", "centred", "reserved", "mu0", "mu1", "mu", "E", "layer_mass", "layer_negative", "ms"]


@pytest.mark.parametrize("T,V,F", [(1, 5, 7), (2, 12, 20), (6, 42, 80), (31, 33, 61)])
@pytest.mark.parametrize("centred", [False, True])
def test_read_out_host_is_the_plug_in_conversion(T, V, F, centred):
    from dots_socp_amd.readout import read_out_host
    from dots_socp_amd.socp import _socp_to_dot, _to_time_centered

    rng = np.random.default_rng(100 * T + V)
    mu, E = rng.standard_normal((T, V)), rng.standard_normal((T + 1, F, 3))
    geom = {"area_vertices": rng.uniform(0.1, 2.0, V), "area_triangles": rng.uniform(0.1, 2.0, F)}
    mu0, mu1 = rng.uniform(0.0, 1.0, V), rng.uniform(0.0, 1.0, V)
    r, dual_scale = 1.7, 0.3
    # the path of the plug-ins: AlmSolver.recovered, then _socp_to_dot, then _to_time_centered
    want = _socp_to_dot({"mu": (r * dual_scale) * mu, "E": (r * dual_scale) * E}, geom)
    if centred:
        _to_time_centered(want, mu0, mu1)
    got_mu, got_E = read_out_host({"mu": mu, "E": E}, r * dual_scale, geom["area_vertices"] / 3.0, geom["area_triangles"], centred, mu0, mu1)
    assert got_mu.shape == (T + 1 if centred else T, V)
    assert np.array_equal(got_mu, want["mu"]) and np.array_equal(got_E, want["E"])
    # no weights, factor 1: the arrays themselves
    same_mu, same_E = read_out_host({"mu": mu, "E": E})
    assert np.array_equal(same_mu, mu) and np.array_equal(same_E, E)
    only_E = read_out_host({"E": E}, 2.0)
    assert only_E[0] is None and np.array_equal(only_E[1], 2.0 * E)


def test_centred_read_out_needs_the_end_points():
    from dots_socp_amd.readout import read_out_host

    with pytest.raises(ValueError):
        read_out_host({"mu": np.zeros((2, 3))}, centred=True)


def test_layer_checks_equal_the_array_checks():
    from dots_socp_amd import evaluate
    from dots_socp_amd.readout import layer_sums_host

    rng = np.random.default_rng(5)
    mu = rng.standard_normal((9, 40)) * 0.05 + 1.0 / 40
    mass, neg = layer_sums_host(mu)
    assert evaluate.mass_conservation_from_layers(mass) == evaluate.check_mass_conservation(mu)
    err, sums = evaluate.negative_mass_from_layers(neg)
    err_ref, sums_ref = evaluate.check_negative_mass(mu)
    assert err == err_ref and np.array_equal(sums, sums_ref)
    assert np.any(sums < 0.0)


def test_plug_ins_take_the_readout_keyword():
    import inspect

    from dots_socp_amd import socp

    for name in ("solver", "solver_raw", "solver_many", "solver_raw_many", "solver_cascade", "solver_raw_cascade"):
        assert inspect.signature(getattr(socp, name)).parameters["readout"].default == "device", name
    with pytest.raises(ValueError):
        socp.solver_raw(4, {}, readout="both")
    assert inspect.signature(socp.solver_socp).parameters["outputs"].default is None


def test_readout_kernels_have_no_private_segment_and_no_spills(tmp_path):
    from dots_socp_amd import _lib
    from test_kernel_resources_cpu import OBJCOPY, READELF, code_objects, kernel_records, short_name

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library is not built")
    if not READELF or not OBJCOPY:
        pytest.skip("llvm-readelf / llvm-objcopy not found")
    recs = {}
    for co in code_objects(_lib.LIB_PATH, str(tmp_path)):
        for r in kernel_records(co):
            recs[short_name(r["name"])] = r
    for name in ("k_readout_mu", "k_readout_E"):
        assert name in recs, sorted(recs)[:5]
        r = recs[name]
        assert int(r["private_segment_fixed_size"]) == 0, (name, r)
        assert int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, (name, r)
