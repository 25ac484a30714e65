"""csrc/admission.h without a GPU: tests/admission_probe.cpp (a stand-alone host program, compiled here with the address and
undefined-behaviour sanitizers) runs every row of the table against every kind of carried work with counters in place of the
runtime.  Its output must equal the table written out below; the table must agree with the replay model of sequence_checks.py; every
exported function that takes a context must have a row or be on the list of those that are not admitted; and dots_api.hip must not
assign a carried field outside the places listed here."""
import os
import re
import subprocess

import pytest

import sequence_checks as sq
from dots_socp_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dots_socp_amd", "csrc")
ERR_ARGUMENT, ERR_STATE = -1, -5
N, A, B = "never", "always", "by_argument"
NEED = {0: N, 1: A, 2: B}


def stale(who):
    return who + ": z_mid was not materialised by the last step (dots_step_flags)"


def stale_source(who):
    return who + ": the source's z_mid was not materialised by its last step (dots_step_flags)"


PALM = "step: DOTS_STEP_PALM needs z_mid of the previous iteration in memory"
# entry: (name in the error texts, access, z_mid read from memory, an unspecified z_mid refused, the refusal's text)
# access: D drops what belongs to the old state or parameters, U the dual arrays are used (a pending division is carried out first),
# S the arrays really change (a slab's KKT halos go stale), F refused while the surface has moved under the iterate
TABLE = {
    "set_params": ("set_params", "D", N, N, None),
    "restart": ("restart", "DS", B, B, stale("restart") + ": no warm start from this iterate"),      # argument: warm
    "penalty_ahead": ("penalty_ahead", "", N, N, None),
    "sync": ("sync", "", N, N, None),
    "stream_wait": ("stream_wait", "", N, N, None),
    "step_flags": ("step_flags", "", N, N, None),
    "step_times": ("step_times", "", N, N, None),
    "geometry_copy": ("geometry_copy", "", N, N, None),
    "front_share_owner": ("front_share", "", N, N, None),
    "step": ("step", "F", B, B, PALM),                          # argument: DOTS_STEP_PALM (the iteration decides itself)
    "step_many": ("step_many", "F", B, B, PALM),
    "slab_stage": ("slab_stage", "U", N, N, None),
    "kkt_combine": ("kkt_combine", "U", N, N, None),
    "objective_combine": ("objective_combine", "U", N, N, None),
    "readout": ("readout", "U", N, N, None),
    "sensitivity": ("sensitivity", "U", N, N, None),
    "flow_map": ("flow_map", "U", N, N, None),
    "flow_push": ("flow_push", "U", N, N, None),
    "flow_trace": ("flow_trace", "U", N, N, None),
    "flow_slide": ("flow_slide", "U", N, N, None),
    "download": ("download", "U", B, B, stale("download")),     # argument: id == Z_MID
    "kkt": ("kkt", "UF", B, B, stale("kkt")),                   # argument: Prim(q, z) in the mask (rebuilt: and the fused sums not taken)
    "kkt_sums": ("kkt_sums", "UF", B, B, stale("kkt")),
    "kkt_sums_device": ("kkt_sums_device", "UF", B, B, stale("kkt")),
    "objective": ("objective", "UF", N, N, None),
    "objective_sums": ("objective_sums", "UF", N, N, None),
    "prolong_time_src": ("prolong_time", "U", A, A, stale_source("prolong_time")),
    "prolong_space_src": ("prolong_space", "U", A, A, stale_source("prolong_space")),
    "transfer_space_src": ("transfer_space", "U", A, A, stale_source("transfer_space")),
    "carry_spacetime_src": ("carry_spacetime", "U", A, A, stale_source("carry_spacetime")),
    "prolong_time": ("prolong_time", "DS", N, N, None),
    "prolong_space": ("prolong_space", "DS", N, N, None),
    "transfer_space": ("transfer_space", "DS", N, N, None),
    "carry_spacetime": ("carry_spacetime", "DS", N, N, None),
    "upload": ("upload", "DUS", B, N, None),                    # argument: id != Z_MID; rebuilt only
    "adjust_penalty": ("adjust_penalty", "DUS", N, N, None),
    "scale_z": ("scale_z", "DUS", A, N, None),
    "scale_arrays": ("scale_arrays", "DUS", A, N, None),
    "move_vertices": ("move_vertices", "DUS", A, N, None),
    "move_vertices_many": ("move_vertices_many", "DUS", A, N, None),
    "run_phase": ("run_phase", "DUF", A, B, stale("phase q_lambda")),      # argument: phase == Q_LAMBDA
    "norm_square": ("norm_square", "DU", B, B, stale("norm_square")),      # argument: id == Z_MID
    "apply_operator": ("apply_operator", "DU", N, N, None),
    "slab_set_buffers": ("slab_set_buffers", "DU", N, N, None),
    "mg_setup": ("mg_setup", "DU", N, N, None),
    "mg_enable": ("mg_enable", "DU", N, N, None),
    "mg_apply": ("mg_apply", "DU", N, N, None),
    "front_setup": ("front_setup", "DU", N, N, None),
    "front_share": ("front_share", "DU", N, N, None),
    "front_enable": ("front_enable", "DU", N, N, None),
    "pcg_windows": ("pcg_windows", "DU", N, N, None),
    "front_launches": ("front_launches", "DU", N, N, None),
    "front_info": ("front_info", "DU", N, N, None),
    "front_pitch": ("front_pitch", "DU", N, N, None),
    "bench_kernel": ("bench_kernel", "DU", B, N, None),         # argument: the kernel reads z_mid
    "laplacian_solve_many": ("laplacian_solve_many", "DU", N, N, None),
    "bench_many": ("bench_many", "DU", N, N, None),
}
NOT_ADMITTED = ("dots_get_params", "dots_array_count", "dots_device_bytes", "dots_slab_elems", "dots_debug_counter", "dots_destroy")
# an exported function -> the rows its contexts are admitted under
ROWS_OF = {"dots_" + e: (e,) for e in TABLE if not e.endswith(("_src", "_owner"))}
ROWS_OF.update({"dots_front_share": ("front_share", "front_share_owner")},
               **{"dots_" + c: (c + "_src", c) for c in ("prolong_time", "prolong_space", "transfer_space", "carry_spacetime")})

DROPPED = ("rhs_ahead", "rhs_ahead_armed", "penalty_armed", "carry_valid", "kkt_fused_valid", "step_path", "deep_path")
STORED, DEFERRED, UNSPECIFIED = 0, 1, 2
# the kinds of carried work: what is set before the call
SITUATIONS = {
    "nothing": {}, "division": {"div": 2.0}, "gathers": {"carry_valid": 1, "step_path": 1024, "deep_path": 1}, "fused_sums": {"kkt_fused_valid": 1},
    "zmid_deferred": {"zmid": DEFERRED}, "zmid_unspecified": {"zmid": UNSPECIFIED}, "rhs_armed": {"rhs_ahead_armed": 1},
    "rhs_ahead_1": {"rhs_ahead": 1}, "rhs_ahead_2": {"rhs_ahead": 2, "ahead_div": 2.0}, "rhs_ahead_3": {"rhs_ahead": 3},
    "rhs_ahead_4": {"rhs_ahead": 4, "div": 2.0}, "penalty_armed": {"penalty_armed": 1}, "halos_fresh": {"halos": 1}, "surface_moved": {"moved": 1},
}


def expected_line(index, entry, arg, situation):
    """What admit, then need_zmid with the argument, do to the situation under the entry's row of TABLE, as the probe prints it."""
    name, access, reads, refuses, text = TABLE[entry]
    k = dict(dict.fromkeys(DROPPED, 0), div=0.0, ahead_div=0.0, zmid=STORED, halos=0, moved=0)
    k.update(SITUATIONS[situation])
    calls, dropped, status, error = "S", [], 0, ""      # the device is selected first
    if "D" in access:
        dropped = [f for f in DROPPED if k[f]]
        k.update(dict.fromkeys(DROPPED, 0))
    if "U" in access and k["div"]:
        calls += "D"
        k["div"] = 0.0
    wanted = lambda need: need == A or (need == B and arg)      # noqa: E731
    if "F" in access and k["moved"]:
        status, error = ERR_STATE, f"dots_{name}: the vertices were moved (dots_move_vertices): the context needs a dots_restart (cold or warm) first"
    elif wanted(refuses) and k["zmid"] == UNSPECIFIED:
        status, error = ERR_STATE, text
    elif wanted(reads) and k["zmid"] == DEFERRED:
        calls += "R"
        k["zmid"] = STORED
    return (f"run {index} arg={int(arg)} {situation} status={status} calls={calls} dropped={','.join(dropped)} after: div={k['div']:g} "
            f"ahead_div={k['ahead_div']:g} zmid={k['zmid']} halos={k['halos']} moved={k['moved']} error={error}")


@pytest.fixture(scope="module")
def probe_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("admission") / "admission_probe")
    cmd = [build.host_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "admission_probe.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_the_probe_does_what_the_table_says(probe_output):
    rows = [ln for ln in probe_output if ln.startswith("row ")]
    want_rows = [f"row {i} {name} access={access} reads={r} refuses={f}" for i, (name, access, r, f, _) in enumerate(TABLE.values())]
    got_rows = [re.sub(r"reads=(\d) refuses=(\d)", lambda m: f"reads={NEED[int(m.group(1))]} refuses={NEED[int(m.group(2))]}", ln) for ln in rows]
    assert got_rows == want_rows      # (the order of TABLE is the order of enum Entry)
    want = []
    for i, (entry, (_, _, reads, refuses, _)) in enumerate(TABLE.items()):
        for arg in ((False, True) if B in (reads, refuses) else (True,)):
            want += [expected_line(i, entry, arg, s) for s in SITUATIONS]
    got = [ln for ln in probe_output if ln.startswith("run ")]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    keeps = "div=2 zmid=1 halos=1 moved=1"      # no drop touches the division, z_mid, the halos or the moved surface
    assert [ln for ln in probe_output if ln.startswith("drop ")] == [
        f"drop change keeps: rhs_ahead=0 rhs_ahead_armed=0 penalty_armed=0 carry_valid=0 kkt_fused_valid=0 step_path=0 deep_path=0 {keeps}",
        f"drop step0 keeps: rhs_ahead=1 rhs_ahead_armed=1 penalty_armed=1 carry_valid=0 kkt_fused_valid=0 step_path=0 deep_path=0 {keeps}",
        f"drop steps23 keeps: rhs_ahead=1 rhs_ahead_armed=1 penalty_armed=1 carry_valid=0 kkt_fused_valid=0 step_path=1 deep_path=1 {keeps}"]


# an operation of sequence_checks.py -> (entry, the argument a "by argument" refusal depends on, as a function of the operation's arguments)
ENTRY_OF = {
    "kkt": ("kkt", lambda a: 1 in a["mask"]), "objective": ("objective", None), "norm_square": ("norm_square", lambda a: a["name"] == "z_mid"),
    "download": ("download", lambda a: a["name"] == "z_mid"), "download_all": ("download", lambda a: True), "apply_operator": ("apply_operator", None),
    "readout": ("readout", None), "sensitivity": ("sensitivity", None), "flow_map": ("flow_map", None), "flow_trace": ("flow_trace", None),
    "flow_push": ("flow_push", None), "flow_slide": ("flow_slide", None), "step": ("step", lambda a: "palm" in a["flags"]), "upload": ("upload", None),
    "adjust_penalty": ("adjust_penalty", None), "set_r": ("set_params", None), "scale_z": ("scale_z", None), "scale_arrays": ("scale_arrays", None),
    "run_phase": ("run_phase", lambda a: a["phase"] == "q_lambda"), "restart_cold": ("restart", lambda a: False), "restart_warm": ("restart", lambda a: True),
}
# (operation as needs_z_mid takes it, its kind): both outcomes of every argument
SAMPLES = ([(("kkt", {"mask": m}), "kkt") for m in sq.MASKS] + [(("download", {"name": n}), "download") for n in ("z_mid", "phi", "beta_mid")]
           + [(("norm_square", {"name": n, "part": p}), "norm_square") for n, p in sq.NORMS] + [(("run_phase", {"phase": p}), "run_phase") for p in sq.PHASES]
           + [(("restart", {"mode": m}), "restart_" + m) for m in ("cold", "warm")] + [(("step", {"flags": f}), "step") for f in ((), ("palm",), ("carry", "kkt_sums"))]
           + [((k, {"name": "z_mid"}), k) for k in ("download_all", "upload", "objective", "apply_operator", "readout", "sensitivity", "adjust_penalty",
                                                    "set_r", "scale_z", "scale_arrays")]
           + [(("flow", {"call": c}), "flow_" + c) for c in ("map", "trace", "push", "slide")])
# The model is stricter than the library in one place: the q_lambda_mult phase reads z_mid from memory as well, and a caller may not
# issue it while z_mid is unspecified, but the library refuses only q_lambda (as it always has).
STRICTER_MODEL = [("run_phase", {"phase": "q_lambda_mult"})]


def test_the_table_agrees_with_the_replay_model():
    assert set(ENTRY_OF) == set(sq.READERS + sq.CHANGERS)
    for kind, (entry, _) in ENTRY_OF.items():
        drops = "D" in TABLE[entry][1]
        if kind in sq.CHANGERS or kind in sq.DROPPERS:
            # (an iteration consumes the carried work itself: its row drops nothing at admission)
            assert drops or kind == "step", kind
        else:
            assert kind in sq.READERS and not drops, kind
    assert {kind for _, kind in SAMPLES} == set(ENTRY_OF)
    differ = []
    for op, kind in SAMPLES:
        entry, argument = ENTRY_OF[kind]
        refuses = TABLE[entry][3]
        refused = refuses == A or (refuses == B and argument(op[1]))
        if refused != bool(sq.needs_z_mid(op)):
            differ.append(op)
    assert differ == STRICTER_MODEL


def test_every_exported_function_with_a_context_is_decided():
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        header = fh.read()
    takes_ctx = set(re.findall(r"^\w[\w ]*?\**(dots_\w+)\((?:const )?dots_ctx \*", header, flags=re.M))
    assert takes_ctx <= set(_lib.EXPORTS) and len(takes_ctx) > 50
    assert not set(NOT_ADMITTED) & set(ROWS_OF)
    assert takes_ctx == set(NOT_ADMITTED) | set(ROWS_OF)
    assert sorted(e for rows in ROWS_OF.values() for e in rows) == sorted(TABLE)
    with open(os.path.join(CSRC, "dots_api.hip")) as fh:
        api = fh.read()
    enum = {e: "E_" + e.upper() for e in TABLE}
    for fn, rows in ROWS_OF.items():
        for e in rows:
            assert re.search(r"\b%s\b" % enum[e], api), (fn, enum[e])      # every row is used
    for fn in NOT_ADMITTED:
        body = re.search(r"^int(?:64_t)? %s\(.*(?:\}|\{\n(?:.*\n)*?\})$" % fn, api, flags=re.M).group(0)
        assert "admit(" not in body and body.count("\n") < 30, fn


FIELDS = ("pending_div", "carry_valid", "kkt_fused_valid", "step_path", "deep_path", "rhs_ahead_armed", "rhs_ahead", "ahead_div", "penalty_armed", "zmid",
          "kkt_halo_fresh", "needs_restart")
# Where dots_api.hip may assign a carried field itself.  The iteration (its plan consumes the launch ahead and the division), the stages
# of a slab, the 3 -> 4 -> 2 confirmation of an anticipated penalty update, the carriers, dots_restart and the move keep their logic;
# the others set what the call itself establishes (a flag armed, z_mid now stored).  Every drop is one of admission.h's named ones.
MAY_ASSIGN = {
    "iteration_before": {"zmid", "pending_div", "ahead_div", "rhs_ahead"}, "slab_stage": {"kkt_halo_fresh"},
    "dots_set_params": {"rhs_ahead", "ahead_div"}, "dots_adjust_penalty": {"pending_div", "rhs_ahead"}, "carry_state": {"pending_div", "zmid"},
    "dots_restart": {"pending_div", "zmid", "needs_restart", "ahead_div"}, "move_holders": {"needs_restart"},
    "dots_penalty_ahead": {"penalty_armed"}, "dots_step_flags": {"rhs_ahead_armed"}, "dots_step_many": {"rhs_ahead_armed"},
    "dots_upload": {"zmid"}, "dots_run_phase": {"zmid"},
}


def test_dots_api_assigns_carried_fields_only_where_listed():
    assign = re.compile(r"(?:\.|->)(%s)\s*(?:[-+|&]?=)(?!=)" % "|".join(FIELDS))
    opens = re.compile(r"^(?:static |inline )*[\w:<>\*&]+ \**(\w+)\(.*\{\s*(?://.*)?$")
    found, fn = {}, None
    with open(os.path.join(CSRC, "dots_api.hip")) as fh:
        for line in fh:
            m = opens.match(line)
            if m:
                fn = m.group(1)
            for f in assign.findall(line.split("//")[0]):
                found.setdefault(fn, set()).add(f)
    assert found == MAY_ASSIGN
