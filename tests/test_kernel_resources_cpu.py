"""The built library's gfx950 code objects, read from their metadata notes: no kernel spills registers to memory and the multi-rhs sweep
kernels are instantiated for exactly the right-hand side counts front_solve_many launches (kernels_front.hip: FRONT_NR_1024_FWD,
FRONT_NR_1024).  A spill shows only as a slowdown; this catches it when the library is built."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from dots_socp_amd import _lib

LLVM_BIN = "/opt/rocm/llvm/bin"
READELF = shutil.which("llvm-readelf", path=LLVM_BIN) or shutil.which("llvm-readelf")
OBJCOPY = shutil.which("llvm-objcopy", path=LLVM_BIN) or shutil.which("llvm-objcopy")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

# kernels allowed a private segment / SGPR spills, with why
PRIVATE_OK = {"k_leaf_tables"}          # setup only: one launch per factorisation
SGPR_SPILL_OK = {"k_fact_panel<0>"}     # k_fact_panel<false>: spills to VGPR lanes, not memory; once per factorisation
# most right-hand sides per launch a 1024-thread workgroup of each sweep kernel takes (kernels_front.hip)
NR_CAP_1024 = {"k_front_fwd": 2, "k_front_bwd": 4, "k_front_leaf_fwd": 4, "k_front_leaf_bwd": 4}
SWEEPS = ("k_front_fwd", "k_front_fwd_rows", "k_front_bwd", "k_front_leaf_fwd", "k_front_leaf_bwd")


def code_objects(lib_path, tmp):
    """the gfx950 entries of every clang offload bundle in the library's .hip_fatbin section"""
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.run([OBJCOPY, "--dump-section", f".hip_fatbin={fatbin}", lib_path, os.path.join(tmp, "lib_copy")], check=True, capture_output=True)
    with open(fatbin, "rb") as fh:
        data = fh.read()
    out = []
    at = data.find(BUNDLE_MAGIC)
    while at >= 0:
        p = at + len(BUNDLE_MAGIC)
        (count,) = struct.unpack_from("<Q", data, p)
        p += 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tlen].decode()
            p += tlen
            if "gfx950" in triple and size > 0:
                path = os.path.join(tmp, f"co{len(out)}.o")
                with open(path, "wb") as fh:
                    fh.write(data[at + off:at + off + size])
                out.append(path)
        at = data.find(BUNDLE_MAGIC, at + 1)
    return out


def kernel_records(code_object):
    """{field: value} per kernel of the object's amdhsa.kernels metadata (top-level fields only)"""
    text = subprocess.run([READELF, "--notes", code_object], check=True, capture_output=True, text=True).stdout
    text = text[text.index("amdhsa.kernels:"):]
    recs = []
    for line in text.splitlines()[1:]:
        if not line.startswith(" "):
            break       # end of the kernel list
        m = re.match(r"^(  - |    )\.([a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            recs.append({})
        recs[-1][m.group(2)] = m.group(3)
    return recs


def short_name(mangled):
    """dots::k_front_fwd<1024, 1, true, 0, 2, 4> as 'k_front_fwd<1024,1,1,0,2,4>' from its Itanium name (template values only)"""
    m = re.match(r"^_ZN4dots(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    base = mangled[m.end():m.end() + n]
    rest = mangled[m.end() + n:]
    if not rest.startswith("I"):
        return base
    args = re.match(r"^I((?:L[ib]\d+E)+)E", rest)
    return base + "<" + ",".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">" if args else base


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library is not built")
    if not READELF or not OBJCOPY:
        pytest.skip("llvm-readelf / llvm-objcopy not found")
    tmp = str(tmp_path_factory.mktemp("fatbin"))
    objs = code_objects(_lib.LIB_PATH, tmp)
    assert objs, "no gfx950 code object in the library"
    out = []
    for co in objs:
        for r in kernel_records(co):
            r["short"] = short_name(r["name"])
            out.append(r)
    return out


def test_code_objects_hold_the_kernels(kernels):
    names = {r["short"].split("<")[0] for r in kernels}
    assert len(kernels) > 100
    assert set(SWEEPS) <= names and "k_leaf_tables" in names and "k_fact_panel" in names


def test_no_kernel_spills_to_memory(kernels):
    bad = []
    for r in kernels:
        if int(r["vgpr_spill_count"]) != 0:
            bad.append((r["short"], "vgpr_spill_count", r["vgpr_spill_count"]))
        if int(r["private_segment_fixed_size"]) != 0 and r["short"].split("<")[0] not in PRIVATE_OK:
            bad.append((r["short"], "private_segment_fixed_size", r["private_segment_fixed_size"]))
        if int(r["sgpr_spill_count"]) != 0 and r["short"] not in SGPR_SPILL_OK:
            bad.append((r["short"], "sgpr_spill_count", r["sgpr_spill_count"]))
    assert not bad, bad


def test_sweep_instantiations_match_the_right_hand_side_caps(kernels):
    """NR is the last template value of every sweep kernel.  A 1024-thread instantiation goes up to its kernel's cap and no higher;
    256- and 512-thread ones (and the row kernel) take 1, 2, 4 and 8."""
    nr_by = {}
    for r in kernels:
        base = r["short"].split("<")[0]
        if base not in SWEEPS:
            continue
        nr = int(r["short"][:-1].split(",")[-1])
        threads = int(r["max_flat_workgroup_size"])
        nr_by.setdefault((base, threads == 1024), set()).add(nr)
    for base in SWEEPS:
        assert nr_by.get((base, False)) == {1, 2, 4, 8}, (base, nr_by.get((base, False)))
    for base, cap in NR_CAP_1024.items():
        want = {nr for nr in (1, 2, 4, 8) if nr <= cap}
        assert nr_by.get((base, True)) == want, (base, nr_by.get((base, True)), cap)
    assert ("k_front_fwd_rows", True) not in nr_by


def test_elementwise_kernels_are_the_lane_bodies_instantiations(kernels):
    """The element-wise half of the iteration is one lane body per step (csrc/kernels_alm.hip: ql_lane, soc_lane, rhs_lane; csrc/kernels_kkt.hip:
    kkt_vertex_body, kkt_triangle_body), instantiated for one and two nodes per lane by these kernels and no others.  A family that splits
    again, or an instantiation a launcher no longer reaches (or reaches anew), changes this set."""
    want = ["k_rhs_modes"]
    want += [f"k_q_lambda_mult_triangle<{z},0>" for z in (0, 1, 2)] + ["k_q_lambda_mult_triangle<0,1>"]                    # <ZMODE, QONLY>
    want += [f"k_q_lambda_mult_triangle2<{z},0>" for z in (0, 1, 2)]
    want += [f"k_q_lambda_mult_carry<{z},{k},{div},{nt}>" for z in (1, 2) for k in (0, 1) for div in (0, 1) for nt in (0, 1)]  # <ZMODE, KKT, DIV, BMNT>
    want += [f"{base}<{v}>" for base in ("k_rhs", "k_slab_pack_iteration", "k_kkt_sums") for v in (0, 1)]                     # <CARRIED>, <CARRIED>, <TWO>
    want += [f"{base}<{c},{div}>" for base in ("k_rhs_modes2", "k_rhs_modes_mfma") for c, div in ((0, 0), (1, 0), (0, 1))]    # <CARRIED, DIV>
    want += [f"k_rhs_modes2_deep<{tp}>" for tp in (8, 16, 32)]
    want += ["k_soc_projection<0,0>", "k_soc_projection<1,0>", "k_soc_projection<1,1>"]                                     # <ONLY_MULTIPLIER, CARRIED>
    families = {w.split("<")[0] for w in want}
    got = sorted(r["short"] for r in kernels if r["short"].split("<")[0] in families)
    assert got == sorted(want)


def test_time_transform_kernels_are_the_ladders_rungs(kernels):
    """The kernels that only transform between time and mode space (csrc/kernels_modes.hip) are the rungs modes_forward, modes_inverse and
    the two time-slab launches choose among, and no others: the forward form straight from memory, the chunked tile form <FWD, NB>, its
    deep form <FWD, NB, pitch>, the MFMA form, the wide body as k_time_modes_wide<pitch> and k_time_modes_windows<pitch, FWD>, and the
    three gathered forms.  An inverse straight from memory that comes back, or a wide body that splits again, changes this set."""
    want = ["k_time_modes", "k_time_modes_tile<1,256>", "k_time_modes_tile<0,256>", "k_time_modes_tile<0,1024>", "k_time_modes_mfma"]
    want += [f"k_time_modes_tile_fast<0,1024,{tp}>" for tp in (8, 16, 32)]
    want += [f"k_time_modes_wide<{tp}>" for tp in (512, 1024)]
    want += [f"k_time_modes_windows<{tp},{fwd}>" for tp in (512, 1024) for fwd in (0, 1)]
    want += ["k_time_modes_fwd_sub", "k_time_modes_fwd_sub_tile", "k_time_modes_inv_gathered_tile"]
    got = sorted(r["short"] for r in kernels if r["short"].startswith("k_time_modes"))
    assert got == sorted(want)


def test_flow_kernels_are_one_tracer_family(kernels):
    """Every trace is a span: the tracer with and without the sliding mode, each bare and with the deposits of 0 .. 4 attributes, and
    the conversion of the sums.  A family that comes back or an instantiation that drops out changes this set."""
    want = ["k_flow_trace", "k_flow_slide", "k_flow_push_finish"]
    want += [f"{base}<{a}>" for base in ("k_flow_trace_push", "k_flow_slide_push") for a in range(5)]
    got = sorted(r["short"] for r in kernels if r["short"].startswith("k_flow"))
    assert got == sorted(want)
