"""csrc/step_choice.h without a GPU: tests/step_choice_probe.cpp (a stand-alone host program, compiled here with the address and
undefined-behaviour sanitizers) prints rhs_choice and ql_choice for every combination of their facts.  Its output must equal the
tables written out below.  A row of a table stands for every combination its pattern matches ('*': the fact does not matter there);
the rows of a table cover every combination exactly once, so the tables are the whole enumeration: 128 combinations of the
right-hand side's seven facts, 6 144 of the twelve of steps 2+3.  The tables were written from the launchers as they were before
the two functions existed (launch_rhs, launch_q_lambda_mult, rhs_divides and ql_divides of kernels_alm.hip, each choosing for
itself); a launch handed a division it cannot apply, which those launchers did not check, is the same choice marked refused.
The source checks at the end hold the context to one stored Dev whose state pointers move in three named places."""
import itertools
import os
import re
import subprocess

import pytest

from dots_socp_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dots_socp_amd", "csrc")

# facts: writes_modes, mfma_ok, tp4, carried, deep_wins, with_soc, pending
RHS_TABLE = """
0**0*00 plain neither path=1 deep=0 divides=0 refused=0
0**0*10 plain neither path=65 deep=0 divides=0 refused=0
0**0*01 plain neither path=1 deep=0 divides=0 refused=1
0**0*11 plain neither path=65 deep=0 divides=0 refused=1
0**1*00 plain carried path=17 deep=0 divides=0 refused=0
0**1*10 plain carried path=81 deep=0 divides=0 refused=0
0**1*01 plain carried path=17 deep=0 divides=0 refused=1
0**1*11 plain carried path=81 deep=0 divides=0 refused=1
1000*00 modes neither path=2 deep=0 divides=0 refused=0
1000*10 modes neither path=66 deep=0 divides=0 refused=0
1000*01 modes neither path=2 deep=0 divides=0 refused=1
1000*11 modes neither path=66 deep=0 divides=0 refused=1
1010*00 modes2 neither path=4 deep=0 divides=1 refused=0
1010*10 modes2 neither path=68 deep=0 divides=1 refused=0
1010*01 modes2 dividing path=36 deep=0 divides=1 refused=0
1010*11 modes2 dividing path=100 deep=0 divides=1 refused=0
1001000 modes neither path=2 deep=0 divides=0 refused=0
1001010 modes neither path=66 deep=0 divides=0 refused=0
1001001 modes neither path=2 deep=0 divides=0 refused=1
1001011 modes neither path=66 deep=0 divides=0 refused=1
1011000 modes2 carried path=20 deep=0 divides=0 refused=0
1011010 modes2 carried path=84 deep=0 divides=0 refused=0
1011001 modes2 carried path=20 deep=0 divides=0 refused=1
1011011 modes2 carried path=84 deep=0 divides=0 refused=1
10*1100 modes2_deep carried path=20 deep=1 divides=0 refused=0
10*1110 modes2_deep carried path=84 deep=1 divides=0 refused=0
10*1101 modes2_deep carried path=20 deep=1 divides=0 refused=1
10*1111 modes2_deep carried path=84 deep=1 divides=0 refused=1
11*0*00 mfma neither path=8 deep=0 divides=1 refused=0
11*0*10 mfma neither path=72 deep=0 divides=1 refused=0
11*0*01 mfma dividing path=40 deep=0 divides=1 refused=0
11*0*11 mfma dividing path=104 deep=0 divides=1 refused=0
11*1*00 mfma carried path=24 deep=0 divides=0 refused=0
11*1*10 mfma carried path=88 deep=0 divides=0 refused=0
11*1*01 mfma carried path=24 deep=0 divides=0 refused=1
11*1*11 mfma carried path=88 deep=0 divides=0 refused=1
"""
# facts: carry_possible, step_carry, step_kkt, zmid_mode (0, 1, 2), fused_present, fused_fit, slab, step_palm, can_defer, tp4, bm_nt, pending
QL_TABLE = """
0**0*****0*0 triangle Z=0 emit=0 defer=0 path=256 divides=0 refused=0
0**0*****0*1 triangle Z=0 emit=0 defer=0 path=256 divides=0 refused=1
0**0*****1*0 triangle2 Z=0 emit=0 defer=0 path=512 divides=0 refused=0
0**0*****1*1 triangle2 Z=0 emit=0 defer=0 path=512 divides=0 refused=1
0**1*****0*0 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=0
0**1*****0*1 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=1
0**1*****1*0 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=0
0**1*****1*1 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=1
0**2*****0*0 triangle Z=2 emit=0 defer=0 path=4352 divides=0 refused=0
0**2*****0*1 triangle Z=2 emit=0 defer=0 path=4352 divides=0 refused=1
0**2*****1*0 triangle2 Z=2 emit=0 defer=0 path=4608 divides=0 refused=0
0**2*****1*1 triangle2 Z=2 emit=0 defer=0 path=4608 divides=0 refused=1
1**0*****0*0 triangle Z=0 emit=0 defer=0 path=256 divides=0 refused=0
1**0*****0*1 triangle Z=0 emit=0 defer=0 path=256 divides=0 refused=1
1**0*****1*0 triangle2 Z=0 emit=0 defer=0 path=512 divides=0 refused=0
1**0*****1*1 triangle2 Z=0 emit=0 defer=0 path=512 divides=0 refused=1
1001**0**0*0 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=0
1001**0**0*1 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=1
1001**0**1*0 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=0
1001**0**1*1 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=1
10110*0**0*0 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=0
10110*0**0*1 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=1
10110*0**1*0 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=0
10110*0**1*1 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=1
1011100*0*00 carry Z=1 emit=0 defer=0 path=3072 divides=1 refused=0
1011100*0*10 carry Z=1 emit=0 defer=0 path=35840 divides=1 refused=0
1011100*0*01 carry Z=1 emit=0 defer=0 path=19456 divides=1 refused=0
1011100*0*11 carry Z=1 emit=0 defer=0 path=52224 divides=1 refused=0
101110001*00 carry Z=2 emit=0 defer=1 path=70656 divides=1 refused=0
101110001*10 carry Z=2 emit=0 defer=1 path=103424 divides=1 refused=0
101110001*01 carry Z=2 emit=0 defer=1 path=87040 divides=1 refused=0
101110001*11 carry Z=2 emit=0 defer=1 path=119808 divides=1 refused=0
101110011*00 carry Z=1 emit=0 defer=0 path=3072 divides=1 refused=0
101110011*10 carry Z=1 emit=0 defer=0 path=35840 divides=1 refused=0
101110011*01 carry Z=1 emit=0 defer=0 path=19456 divides=1 refused=0
101110011*11 carry Z=1 emit=0 defer=0 path=52224 divides=1 refused=0
1011110*0*00 carry Z=1 emit=2 defer=0 path=11264 divides=1 refused=0
1011110*0*10 carry Z=1 emit=2 defer=0 path=44032 divides=1 refused=0
1011110*0*01 carry Z=1 emit=2 defer=0 path=27648 divides=1 refused=0
1011110*0*11 carry Z=1 emit=2 defer=0 path=60416 divides=1 refused=0
101111001*00 carry Z=2 emit=2 defer=1 path=78848 divides=1 refused=0
101111001*10 carry Z=2 emit=2 defer=1 path=111616 divides=1 refused=0
101111001*01 carry Z=2 emit=2 defer=1 path=95232 divides=1 refused=0
101111001*11 carry Z=2 emit=2 defer=1 path=128000 divides=1 refused=0
101111011*00 carry Z=1 emit=2 defer=0 path=11264 divides=1 refused=0
101111011*10 carry Z=1 emit=2 defer=0 path=44032 divides=1 refused=0
101111011*01 carry Z=1 emit=2 defer=0 path=27648 divides=1 refused=0
101111011*11 carry Z=1 emit=2 defer=0 path=60416 divides=1 refused=0
10*1**1**0*0 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=0
10*1**1**0*1 triangle Z=1 emit=0 defer=0 path=2304 divides=0 refused=1
10*1**1**1*0 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=0
10*1**1**1*1 triangle2 Z=1 emit=0 defer=0 path=2560 divides=0 refused=1
1101**0*0*00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
1101**0*0*10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
1101**0*0*01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
1101**0*0*11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
1101**001*00 carry Z=2 emit=1 defer=1 path=70656 divides=1 refused=0
1101**001*10 carry Z=2 emit=1 defer=1 path=103424 divides=1 refused=0
1101**001*01 carry Z=2 emit=1 defer=1 path=87040 divides=1 refused=0
1101**001*11 carry Z=2 emit=1 defer=1 path=119808 divides=1 refused=0
1101**011*00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
1101**011*10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
1101**011*01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
1101**011*11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
11110*0*0*00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
11110*0*0*10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
11110*0*0*01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
11110*0*0*11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
11110*001*00 carry Z=2 emit=1 defer=1 path=70656 divides=1 refused=0
11110*001*10 carry Z=2 emit=1 defer=1 path=103424 divides=1 refused=0
11110*001*01 carry Z=2 emit=1 defer=1 path=87040 divides=1 refused=0
11110*001*11 carry Z=2 emit=1 defer=1 path=119808 divides=1 refused=0
11110*011*00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
11110*011*10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
11110*011*01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
11110*011*11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
1111100*0*00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
1111100*0*10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
1111100*0*01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
1111100*0*11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
111110001*00 carry Z=2 emit=1 defer=1 path=70656 divides=1 refused=0
111110001*10 carry Z=2 emit=1 defer=1 path=103424 divides=1 refused=0
111110001*01 carry Z=2 emit=1 defer=1 path=87040 divides=1 refused=0
111110001*11 carry Z=2 emit=1 defer=1 path=119808 divides=1 refused=0
111110011*00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
111110011*10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
111110011*01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
111110011*11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
1111110*0*00 carry Z=1 emit=3 defer=0 path=11264 divides=1 refused=0
1111110*0*10 carry Z=1 emit=3 defer=0 path=44032 divides=1 refused=0
1111110*0*01 carry Z=1 emit=3 defer=0 path=27648 divides=1 refused=0
1111110*0*11 carry Z=1 emit=3 defer=0 path=60416 divides=1 refused=0
111111001*00 carry Z=2 emit=3 defer=1 path=78848 divides=1 refused=0
111111001*10 carry Z=2 emit=3 defer=1 path=111616 divides=1 refused=0
111111001*01 carry Z=2 emit=3 defer=1 path=95232 divides=1 refused=0
111111001*11 carry Z=2 emit=3 defer=1 path=128000 divides=1 refused=0
111111011*00 carry Z=1 emit=3 defer=0 path=11264 divides=1 refused=0
111111011*10 carry Z=1 emit=3 defer=0 path=44032 divides=1 refused=0
111111011*01 carry Z=1 emit=3 defer=0 path=27648 divides=1 refused=0
111111011*11 carry Z=1 emit=3 defer=0 path=60416 divides=1 refused=0
11*1**1***00 carry Z=1 emit=1 defer=0 path=3072 divides=1 refused=0
11*1**1***10 carry Z=1 emit=1 defer=0 path=35840 divides=1 refused=0
11*1**1***01 carry Z=1 emit=1 defer=0 path=19456 divides=1 refused=0
11*1**1***11 carry Z=1 emit=1 defer=0 path=52224 divides=1 refused=0
10*2*****0*0 triangle Z=2 emit=0 defer=0 path=4352 divides=0 refused=0
10*2*****0*1 triangle Z=2 emit=0 defer=0 path=4352 divides=0 refused=1
10*2*****1*0 triangle2 Z=2 emit=0 defer=0 path=4608 divides=0 refused=0
10*2*****1*1 triangle2 Z=2 emit=0 defer=0 path=4608 divides=0 refused=1
11*2******00 carry Z=2 emit=1 defer=0 path=5120 divides=1 refused=0
11*2******10 carry Z=2 emit=1 defer=0 path=37888 divides=1 refused=0
11*2******01 carry Z=2 emit=1 defer=0 path=21504 divides=1 refused=0
11*2******11 carry Z=2 emit=1 defer=0 path=54272 divides=1 refused=0
"""
RHS_DIGITS = ["01"] * 7
QL_DIGITS = ["01"] * 3 + ["012"] + ["01"] * 8
# the kernel each name of the probe stands for (kernels_alm.hip)
KERNEL = {"mfma": "k_rhs_modes_mfma", "modes2_deep": "k_rhs_modes2_deep", "modes2": "k_rhs_modes2", "modes": "k_rhs_modes", "plain": "k_rhs",
          "carry": "k_q_lambda_mult_carry", "triangle2": "k_q_lambda_mult_triangle2", "triangle": "k_q_lambda_mult_triangle"}


def expand(table, digits):
    """{facts: outcome} of every combination the rows match; every combination is matched by exactly one row"""
    out = {}
    for row in table.strip().splitlines():
        pattern, outcome = row.split(" ", 1)
        assert len(pattern) == len(digits), row
        for combo in itertools.product(*[d if p == "*" else p for p, d in zip(pattern, digits)]):
            facts = "".join(combo)
            assert facts not in out, (row, facts)
            out[facts] = outcome
    assert sorted(out) == sorted("".join(c) for c in itertools.product(*digits))
    return out


@pytest.fixture(scope="module")
def probe_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_choice") / "step_choice_probe")
    cmd = [build.host_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "step_choice_probe.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def rows_of(probe_output, which):
    return dict(ln.split(" ", 2)[1:] for ln in probe_output if ln.startswith(which + " "))


def test_the_probe_prints_the_tables(probe_output):
    for which, table, digits, n in (("rhs", RHS_TABLE, RHS_DIGITS, 128), ("ql", QL_TABLE, QL_DIGITS, 6144)):
        want, got = expand(table, digits), rows_of(probe_output, which)
        assert len(want) == n and len([ln for ln in probe_output if ln.startswith(which + " ")]) == n
        assert sorted(got) == sorted(want)
        for facts in want:
            assert got[facts] == want[facts], (which, facts)


def dividing_kernels():
    """kernel -> its template has a DIV argument (kernels_alm.hip)"""
    with open(os.path.join(CSRC, "kernels_alm.hip")) as fh:
        src = fh.read()
    out = {}
    for m in re.finditer(r"^(template <[^\n]*>\n)?__global__ [^\n]*?void (k_\w+)\(", src, flags=re.M):
        out[m.group(2)] = "bool DIV" in (m.group(1) or "")
    return out


def test_divides_goes_with_the_kernels_that_can_and_the_rest_is_refused(probe_output):
    can = dividing_kernels()
    assert {k for k in KERNEL.values() if can[k]} == {"k_rhs_modes_mfma", "k_rhs_modes2", "k_q_lambda_mult_carry"}
    field = lambda outcome, name: int(re.search(r"\b%s=(\d+)" % name, outcome).group(1))      # noqa: E731
    for which in ("rhs", "ql"):
        for facts, outcome in rows_of(probe_output, which).items():
            words = outcome.split()
            kernel, pending = KERNEL[words[0]], facts[-1] == "1"
            # the right-hand-side kernels have CARRIED and DIV, and the launcher never instantiates both: the carried variant cannot divide
            expected = can[kernel] and not (which == "rhs" and words[1] == "carried")
            assert field(outcome, "divides") == int(expected), (which, facts, outcome)
            assert field(outcome, "refused") == int(pending and not expected), (which, facts, outcome)
            div_bit = _lib.STEP_PATH["rhs_div" if which == "rhs" else "ql_div"]
            assert bool(field(outcome, "path") & div_bit) == (pending and expected), (which, facts, outcome)
            if which == "rhs":
                assert (words[1] == "dividing") == (pending and expected), (facts, outcome)


def test_the_path_bits_are_the_python_side_s(probe_output):
    (line,) = [ln for ln in probe_output if ln.startswith("bits ")]
    bits = {k: int(v) for k, v in (w.split("=") for w in line.split()[1:])}
    assert {k: bits[k] for k in _lib.STEP_PATH} == _lib.STEP_PATH
    assert bits["ql_z_shift"] == _lib.STEP_PATH_QL_Z_SHIFT
    assert {"rhs": bits["deep_rhs"], "inverse": bits["deep_inverse"]} == _lib.DEEP_PATH
    assert set(bits) == set(_lib.STEP_PATH) | {"ql_z_shift", "deep_rhs", "deep_inverse"}


# ---- the source: one stored Dev, its state pointers moved in three named places ----
STATE_POINTERS = ("zf", "ze", "lamc", "B", "bm", "zm", "B_st", "bm_st")
OPENS = re.compile(r"^\s*(?:static |inline |explicit )*[\w:<>\*&]+ \**(\w+)\(.*\{\s*(?://.*)?$")


def csrc_files():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))


def code_lines(path):
    """(function the line is in, the line without its comment) of a source file; inside struct Ctx the function names are its members'"""
    fn = None
    with open(path) as fh:
        for line in fh:
            m = OPENS.match(line)
            if m and m.group(1) not in ("if", "for", "while", "switch"):
                fn = m.group(1)
            yield fn, line.split("//")[0]


def test_a_context_stores_one_dev():
    with open(os.path.join(CSRC, "dots_dev.h")) as fh:
        body = re.search(r"^struct Ctx \{\n(.*?)^\};", fh.read(), flags=re.M | re.S).group(1)
    assert re.findall(r"^\s*Dev\s+(\w+)", body, flags=re.M) == ["d"]
    assert not re.search(r"\bDev\s*[\*&]?\s*\w+\s*(?:\{\}|=[^=]|;)", body.replace("Dev d{};", "", 1))
    for path in csrc_files():
        with open(path) as fh:
            assert "Dev keep" not in fh.read(), path


def test_the_penalty_is_assigned_where_the_caller_sets_it():
    where = set()
    for path in csrc_files():
        for fn, code in code_lines(path):
            if re.search(r"\bprm\.r\s*[-+*/]?=(?!=)|\bprm\s*=(?!=)", code):
                where.add(fn)
    assert where and where <= {"dots_set_params", "dots_adjust_penalty", "dots_restart"}, where


def test_the_state_pointers_move_in_build_and_the_two_swaps():
    names = "|".join(STATE_POINTERS)
    where = {}
    for path in csrc_files():
        aliases, last_fn = set(), None
        in_ctx = False
        for fn, code in code_lines(path):
            if code.startswith("struct Ctx {"):
                in_ctx = True
            elif code.startswith("};"):
                in_ctx = False
            if fn != last_fn:
                aliases, last_fn = set(), fn
            m = re.search(r"(?<!const )Dev &(\w+) = c->d;", code)
            if m:
                aliases.add(m.group(1))      # a writable name for the context's Dev
            owners = ["c->d"] + sorted(aliases) + (["d"] if in_ctx else [])
            who = "(?:%s)" % "|".join(r"(?<![\w.>])" + re.escape(o) for o in owners)
            hits = re.findall(r"%s\.(%s)\s*=(?!=)" % (who, names), code) + re.findall(r"swap\(\s*%s\.(%s)\b" % (who, names), code)
            hits += re.findall(r"swap\([^()]*,\s*%s\.(%s)\b" % (who, names), code) + re.findall(r"&%s\.(%s)\b" % (who, names), code)
            for h in hits:
                where.setdefault(fn, set()).add(h)
    assert where == {"build": set(STATE_POINTERS), "swap_ahead_projection": {"zf", "ze", "lamc"},
                     "swap_deferred_zmid": {"B", "bm", "zm", "B_st", "bm_st"}}
