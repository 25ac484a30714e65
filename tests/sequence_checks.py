"""Random call sequences against the fp64 oracle and an eager twin (test_sequence_checks_cpu.py, test_hip_sequences.py; plain numpy,
TEST INFRASTRUCTURE).

A context carries deferred work between calls (a penalty division not yet applied, per-corner gathers carried from steps 2+3, KKT sums
left as partial sums, a z_mid that is unspecified or still to be rebuilt, a right-hand side launched ahead, an armed penalty decision),
and every entry point decides which of it to flush, keep or drop.  The header promises that results never depend on any of it.  Here:

``make_sequence``  a sequence of operations as plain data ``(name, arguments)``: episodes that set a SITUATION up (what is pending
                   when a call arrives, told from the sequence alone) and then issue one reader or one state-changing call into it.
                   The committed sequences (``SEEDS``) are CONSTRUCTED, not sampled: one fixed list of episodes that walks the table
                   ``REQUIRED`` of (situation, operation) pairs, packed into sequences, the seed being the index of a sequence; a
                   fixed picker deals out flags, masks and names in turn.  Only seeds beyond ``SEEDS`` draw their episodes at random;
``situations``     what held when every operation of a sequence was issued; ``coverage``: the (situation, kind) pairs reached;
``replay``         the sequence on three players: ``lazy`` (the library's defaults and the flags the sequence names), ``eager`` (a
                   context that defers nothing: no hints, no penalty_ahead; it is downloaded after every operation) and the fp64 oracle,
                   loaded from ``eager``'s state before each operation and compared with ``eager``'s state after it.  Everything the
                   sequence reads must come out of ``lazy`` and ``eager`` with the same bits, and so must the twelve arrays at the end;
``shrink``         greedy removal of single operations while a predicate still fails."""
import math

import numpy as np

import step_checks as sc
from mode_checks import MARGIN
from dots_socp_amd import _lib, flow, readout, sensitivity
from dots_socp_amd.control import AdjustAdmmParam

O = sc.O
STATE, DUAL = sc.STATE, sc.DUAL
ERR_ARGUMENT, ERR_STATE = _lib.ERR_ARGUMENT, _lib.ERR_STATE
FLAGS = ("skip_z_mid", "palm", "rhs_ahead", "carry", "kkt_sums", "timed")
MASKS = ((0,), (1,), (2,), (3,), (4,), (5,), (6,), (0, 1, 2, 3), (0, 1, 2, 3, 6), (0, 1, 2, 3, 4, 5, 6), (4, 5))
FUSED = frozenset((0, 1, 2, 3, 6))            # the conditions a read may take from the sums a kkt_sums step left
FUSED_TOL = 1e-12                             # ... and how far such a read may be from the stand-alone one (test_kkt_sums_formed_by_steps_2_and_3)
NORM_TOL = {("phi", 0): 1e-13, ("phi", 1): 1e-12, ("phi", 2): 1e-12, ("mu", 0): 1e-13, ("E", 0): 1e-13, ("z_mid", 0): 1e-13,
            ("beta_mid", 0): 1e-13}          # test_kkt_objective_norms_a10_a11_a12 (z_mid: beta_mid's kernel and weights)
NORMS = tuple(NORM_TOL)
PHASES = ("laplacian", "soc_projection", "q_lambda_mult", "q_lambda")
OPERATORS = {"grad_time": "phi", "div_space": "B", "decouple": "B", "decouple_adjoint": "beta_mid"}      # operator -> the state array it is fed
WARM_FACTORS = (1.1, 0.9, 1.2, 0.8)
DROP = 1.25                                   # the caller's factor is the anticipated one times this: the launch ahead is dropped
POLICY = dict(tol=1e-4, is_org_kkt=False)     # the driver's default tol: none of the states here passes it
FLOOR, CROSSINGS, PARTICLES = 0.3, 4, 3
LENGTH = 16

# ---- situations --------------------------------------------------------------------------------------------------------------------
DIV, CARRY, KSUM, SKIP, AHEAD, ARMED, MULTI = "div", "carry", "kkt_sums", "skip", "ahead", "armed", "multi"
SINGLE = (DIV, CARRY, KSUM, SKIP, AHEAD, ARMED)
READERS = ("kkt", "objective", "norm_square", "download", "download_all", "apply_operator", "readout", "sensitivity", "flow_map", "flow_trace",
           "flow_push", "flow_slide")
CHANGERS = ("step", "upload", "adjust_penalty", "set_r", "scale_z", "scale_arrays", "run_phase", "restart_cold", "restart_warm")
MULTI_KINDS = ("readout", "sensitivity", "flow_map", "restart_warm", "restart_cold", "download_z_mid", "kkt_all", "confirm", "drop")
DROPPERS = ("norm_square", "apply_operator")      # they leave the state alone, but the library treats them as calls that change it (the header)
ONLY_REFUSED = ("download_all", "restart_warm")   # what reads z_mid whatever its arguments: while z_mid is unspecified it can only be refused
REQUIRED = frozenset([(s, k) for s in SINGLE for k in READERS + CHANGERS if not (s == SKIP and k in ONLY_REFUSED)] + [(MULTI, k) for k in MULTI_KINDS]
                     + [(ARMED, "confirm"), (ARMED, "drop")]
                     + [(SKIP, "refuse_" + w) for w in ("download_z_mid", "download_all", "kkt_1", "restart_warm", "palm_step")])
REFUSALS = {"download_z_mid": (ERR_STATE, False), "download_all": (ERR_STATE, False), "kkt_1": (ERR_STATE, False), "restart_warm": (ERR_STATE, False),
            "palm_step": (ERR_STATE, False), "flags_palm_skip": (ERR_ARGUMENT, True),
            "flags_palm_ahead": (ERR_ARGUMENT, True)}      # what -> (status, from both contexts)


def kinds(op):
    """The kinds an operation counts as in ``coverage``."""
    name, a = op
    if name == "kkt":
        return {"kkt"} | ({"kkt_all"} if len(a["mask"]) == 7 else set())
    if name == "download":
        return {"download"} | ({"download_z_mid"} if a["name"] == "z_mid" else set())
    if name == "adjust_penalty":
        return {"adjust_penalty"} | ({a["how"]} if a.get("how") in ("confirm", "drop") else set())
    if name == "restart":
        return {"restart_" + a["mode"]}
    if name == "flow":
        return {"flow_" + a["call"]}
    if name == "refuse":
        return {"refuse_" + a["what"]}
    return {name}


def needs_z_mid(op):
    """The operation reads z_mid from memory: the caller may not issue it while z_mid is unspecified."""
    name, a = op
    return ((name == "kkt" and 1 in a["mask"]) or (name == "download" and a["name"] == "z_mid") or name == "download_all"
            or (name == "norm_square" and a["name"] == "z_mid") or (name == "run_phase" and a["phase"] in ("q_lambda", "q_lambda_mult"))
            or (name == "restart" and a["mode"] == "warm") or (name == "step" and "palm" in a["flags"]))


class Shadow:
    """The caller's side of the documented rules: z_mid is unspecified after a step with skip_z_mid until a step without it, an upload
    of it, the projection phase or a cold restart."""

    def __init__(self):
        self.stale = False

    def legal(self, op):
        name, a = op
        if name == "refuse":
            return self.stale or REFUSALS[a["what"]][1]
        if name == "step" and "palm" in a["flags"] and ("skip_z_mid" in a["flags"] or "rhs_ahead" in a["flags"]):
            return False
        return not (self.stale and needs_z_mid(op))

    def take(self, op):
        name, a = op
        if name == "step":
            self.stale = "skip_z_mid" in a["flags"]
        elif (name == "upload" and a["name"] == "z_mid") or (name == "run_phase" and a["phase"] == "soc_projection") or \
                (name == "restart" and a["mode"] == "cold"):
            self.stale = False


def legal(sequence):
    sh = Shadow()
    for op in sequence:
        if not sh.legal(op):
            return False
        sh.take(op)
    return True


def stale_at_end(sequence):
    sh = Shadow()
    for op in sequence:
        sh.take(op)
    return sh.stale


def situations(sequence):
    """For every operation the set of situations that held when it was issued, from the sequence alone and the header's rules: SKIP
    while z_mid is unspecified (``Shadow``); AHEAD and ARMED until a call that changes the state or the parameters, which
    dots_norm_square and dots_apply_operator count as (``DROPPERS``)."""
    out = []
    div, last, ahead, armed, sh = False, None, 0, 0, Shadow()
    for op in sequence:
        name, a = op
        now = set()
        if div:
            now.add(DIV)
        if last is not None and last[0] == "step":
            f = last[1]["flags"]
            if "carry" in f and "palm" not in f:
                now.add(CARRY)
            if "kkt_sums" in f and "skip_z_mid" not in f:
                now.add(KSUM)
        if sh.stale:
            now.add(SKIP)
        if ahead == 2:
            now.add(AHEAD)
        if armed == 2:
            now.add(ARMED)
        if len(now) >= 2:
            now.add(MULTI)
        out.append(frozenset(now))
        sh.take(op)
        if name == "step":
            div = False
            ahead = 1 if "rhs_ahead" in a["flags"] else 0
            armed = 1 if armed == 1 else 0
        elif name == "kkt":
            div = False
            ahead = 2 if ahead else 0
            armed = 2 if armed == 2 or (armed == 1 and set(a["mask"]) >= {0, 1, 2, 3}) else armed
        elif name == "penalty_ahead":
            armed = 1
        elif name in ("refuse",):
            pass
        elif name == "set_r":
            ahead = armed = 0      # (set_params neither reads nor writes the dual arrays: a division stays requested)
        elif name in CHANGERS or name == "restart" or name in DROPPERS:
            ahead = armed = 0
            div = name == "adjust_penalty"
        else:      # the other readers carry a division out
            div = False
        last = op
    return out


def fused_reads(sequence):
    """For every operation: it is a KKT read that may take the sums a kkt_sums step left (the header: a read whose mask lies within
    FUSED, after such a step and before any call that changes the state or the parameters -- ``DROPPERS`` included; reads in between
    keep the sums)."""
    out, live = [], False
    for name, a in sequence:
        out.append(name == "kkt" and live and set(a["mask"]) <= FUSED)
        if name == "step":
            live = "kkt_sums" in a["flags"] and "skip_z_mid" not in a["flags"]
        elif name in CHANGERS or name == "restart" or name in DROPPERS:
            live = False
    return out


def cancelling_reads(sequence):
    """For every operation: it is a KKT read of Dual(beta) on a state on which that residual vanishes but for rounding.  scale_z SETS
    mu = sz (beta_fst - beta_end) and E = -L^T beta_mid, a cold restart zeroes them all, and from there on the iteration keeps both
    identities (the multiplier update moves the two sides alike; the other phases do not touch them; a penalty division divides all
    five arrays alike).  An upload, scale_arrays or a warm restart (another factor for (mu, E) than for the betas) ends it."""
    out, live = [], False
    for name, a in sequence:
        out.append(name == "kkt" and live and 3 in a["mask"])
        if name == "scale_z" or (name == "restart" and a["mode"] == "cold"):
            live = True
        elif name in ("upload", "scale_arrays", "restart"):
            live = False
    return out


def coverage(sequences):
    out = set()
    for seq in sequences:
        for op, sits in zip(seq, situations(seq)):
            for k in kinds(op):
                out.update((s, k) for s in sits)
    return out


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def step(*flags, wait=False):
    return ("step", {"flags": sorted(flags), "wait": bool(wait)})


class Picker:
    """The generator's choices: coin flips from the seed, and for what a kind leaves open (which mask, array, phase) the next of the
    candidates in turn, so that all of them get their call."""

    def __init__(self, seed):
        self.rng, self.turn = np.random.default_rng(seed), {}

    def integers(self, n):
        return int(self.rng.integers(n))

    def pick(self, key, xs):
        i = self.turn.get(key, 0)
        self.turn[key] = i + 1
        return xs[i % len(xs)]


def _target(kind, rng, sits=()):
    """One operation of ``kind`` into the situations ``sits``; the picker chooses what the kind leaves open."""
    pick = lambda xs: rng.pick(kind, list(xs))      # noqa: E731
    stale = SKIP in sits
    if kind == "kkt":
        return ("kkt", {"mask": list(pick([m for m in MASKS if not (stale and 1 in m)]))})
    if kind == "kkt_all":
        return ("kkt", {"mask": list(range(7))})
    if kind == "objective":
        return ("objective", {})
    if kind == "norm_square":
        name, part = pick([n for n in NORMS if not (stale and n[0] == "z_mid")])
        return ("norm_square", {"name": name, "part": part})
    if kind == "download":
        return ("download", {"name": pick(DUAL if DIV in sits else [k for k in STATE if not (stale and k == "z_mid")])})
    if kind == "download_z_mid":
        return ("download", {"name": "z_mid"})
    if kind == "download_all":
        return ("download_all", {})
    if kind == "apply_operator":
        return ("apply_operator", {"op": pick(sorted(OPERATORS))})
    if kind == "readout":
        return ("readout", {"centred": bool(rng.integers(2)), "weighted": bool(rng.integers(2)), "factor": 0.37})
    if kind == "sensitivity":
        return ("sensitivity", {"factor_phi": 1.3, "factor_mu": 0.7})
    if kind.startswith("flow_"):
        return ("flow", {"call": kind[5:], "seed": int(rng.integers(1 << 16)), "backward": bool(rng.integers(2))})
    if kind == "step":
        if not stale and rng.integers(5) == 0:
            return step("palm", *(["carry"] if rng.integers(2) else []), wait=rng.integers(4) == 0)
        extra = [f for f in ("carry", "kkt_sums", "timed", "rhs_ahead") if rng.integers(3) == 0]
        return step(*extra, wait=rng.integers(4) == 0)
    if kind == "upload":
        return ("upload", {"name": pick(("B", "E", "beta_mid") if CARRY in sits else ("mu", "beta_mid") if DIV in sits else STATE)})
    if kind == "adjust_penalty":
        return ("adjust_penalty", {"f": pick((sc.FACTOR, 0.6, 1.3)), "how": "given"})
    if kind in ("confirm", "drop"):
        return ("adjust_penalty", {"f": sc.FACTOR, "how": kind})      # (f: what a replay without the KKT read before it falls back to)
    if kind == "set_r":
        return ("set_r", {"f": pick((1.4, 0.7))})
    if kind == "scale_z":
        return ("scale_z", {"f": pick((0.8, 1.25))})
    if kind == "scale_arrays":
        return ("scale_arrays", {"names": sorted({pick(STATE), pick(DUAL)}), "f": 0.9})
    if kind == "run_phase":
        return ("run_phase", {"phase": pick([p for p in PHASES if not (stale and p in ("q_lambda", "q_lambda_mult"))])})
    if kind in ("restart_cold", "restart_warm"):
        return ("restart", {"mode": kind[8:], "swap": bool(rng.integers(2))})
    raise KeyError(kind)


def _setup(sit, rng, kind):
    """The operations that bring the situation ``sit`` about for the next one."""
    some = lambda *fl: [f for f in fl if rng.integers(2)]      # noqa: E731
    wait = bool(rng.integers(4) == 0)
    if sit == DIV:
        return [("adjust_penalty", {"f": sc.FACTOR if rng.integers(2) else 0.6, "how": "given"})]
    if sit == CARRY:
        return [step("carry", *some("timed", "rhs_ahead"), wait=wait)]
    if sit == KSUM:
        return [step("kkt_sums", *some("timed"), wait=wait)]
    if sit == SKIP:
        return [step("skip_z_mid", *some("timed", "carry"), wait=wait)]
    if sit == AHEAD:
        return [step("rhs_ahead", *some("carry", "kkt_sums"), wait=False), ("kkt", {"mask": list(rng.pick("ahead", MASKS))})]
    if sit == ARMED:
        return [step(*some("kkt_sums", "timed"), wait=False), ("penalty_ahead", {}), ("kkt", {"mask": [0, 1, 2, 3] if rng.integers(2) else [0, 1, 2, 3, 6]})]
    raise KeyError(sit)


def _multi_setup(kind, rng):
    if kind in ("confirm", "drop"):      # armed, and a right-hand side ahead
        return [step("rhs_ahead", wait=False), ("penalty_ahead", {}), ("kkt", {"mask": [0, 1, 2, 3]})]
    if kind in ("sensitivity", "restart_cold"):      # z_mid unspecified and a division requested
        return [step("skip_z_mid", "carry", wait=False), ("adjust_penalty", {"f": sc.FACTOR, "how": "given"})]
    if kind == "flow_map":
        return [step("skip_z_mid", "carry", wait=False)]
    return [step("carry", "kkt_sums", *(["rhs_ahead"] if rng.integers(2) else []), wait=False)]      # gathers carried, sums fused, z_mid deferred


def _episodes():
    """Every pair of REQUIRED as one episode, readers of a lasting situation sharing its setup; then the combinations the header's
    contract is thinnest on, as explicit chains."""
    eps, picker = [], Picker(20260)

    def rng():
        return picker

    for sit in (DIV, CARRY, KSUM):      # gone after one call: one setup per target
        for kind in READERS + CHANGERS:
            r = rng()
            eps.append(_setup(sit, r, kind) + [_target(kind, r, (sit,))])
    for sit in (SKIP, AHEAD, ARMED):    # lasts over readers: up to four of them and then one call that ends it, per setup
        enders = tuple(k for k in CHANGERS if not (sit == SKIP and k in ONLY_REFUSED))
        if sit == SKIP:                 # (nothing but a step, an upload of z_mid, the projection or a cold restart ends it)
            readers = [k for k in READERS if k not in ONLY_REFUSED]
        else:
            readers, enders = [k for k in READERS if k not in DROPPERS], DROPPERS + enders
        enders = list(enders)
        while readers or enders:
            r = rng()
            group, readers = readers[:4], readers[4:]
            tail, enders = enders[:1], enders[1:]
            eps.append(_setup(sit, r, (group + tail)[0]) + [_target(k, r, (sit,)) for k in group + tail])
    for kind in ("confirm", "drop"):
        r = rng()
        eps.append(_setup(ARMED, r, kind) + [_target(kind, r, (ARMED,)), step(wait=False), ("kkt", {"mask": [4, 5]})])
    for kind in MULTI_KINDS:
        r = rng()
        eps.append(_multi_setup(kind, r) + [_target(kind, r, (MULTI,) + ((SKIP,) if kind in ("sensitivity", "restart_cold", "flow_map") else ()))])
    for what in REFUSALS:
        r = rng()
        eps.append([step("skip_z_mid", *(["carry"] if r.integers(2) else []), wait=False), ("refuse", {"what": what}), step(wait=False)])
    # Dual(beta) where scale_z has just set mu and E to what makes it vanish, and after a penalty division on top
    eps.append([step(wait=False), ("scale_z", {"f": 0.8}), ("kkt", {"mask": [3]}), ("adjust_penalty", {"f": 1.3, "how": "given"}),
                ("kkt", {"mask": [0, 1, 2, 3]})])
    # a division that rode in a carried step (recorded with the deferred z_mid), gathers carried, a right-hand side ahead: all at once
    for kind in ("download_z_mid", "readout", "flow_trace", "restart_warm", "norm_square", "run_phase", "scale_z", "upload"):
        r = rng()
        eps.append([("adjust_penalty", {"f": sc.FACTOR, "how": "given"}), step("carry", "kkt_sums", "rhs_ahead", wait=False),
                    ("kkt", {"mask": [0, 2, 3]}), _target(kind, r, (CARRY,)), step("carry", wait=False)])
    # every array downloaded, the first of each three with gathers carried, sums fused and z_mid deferred
    for i in range(0, 12, 4):
        eps.append([step("carry", "kkt_sums", wait=False)] + [("download", {"name": k}) for k in STATE[i:i + 4]])
    # is_palm's step 0 reads the z_mid nobody asked for
    eps.append([step("carry", "kkt_sums", wait=False), step("palm", wait=False), ("download", {"name": "z_mid"})])
    # what the planted defects of test_sequence_checks_cpu.py need behind the call: the next read or step shows what was kept
    eps.append([step("kkt_sums", wait=False), ("run_phase", {"phase": "q_lambda"}), ("kkt", {"mask": [0, 1, 2, 3, 6]})])
    eps.append([step("rhs_ahead", wait=False), ("kkt", {"mask": [0, 2, 3]}), ("set_r", {"f": 1.4}), step(wait=False), ("download", {"name": "phi"})])
    eps.append([step("carry", wait=False), ("upload", {"name": "beta_mid"}), step("carry", wait=False), ("download", {"name": "z_fst"})])
    eps.append([step(wait=False), ("adjust_penalty", {"f": sc.FACTOR, "how": "given"}), ("adjust_penalty", {"f": 0.6, "how": "given"}),
                ("download", {"name": "beta_mid"})])
    eps.append([step(wait=False), ("adjust_penalty", {"f": sc.FACTOR, "how": "given"}), ("restart", {"mode": "cold", "swap": True}), step(wait=False),
                step("carry", wait=False)])
    return eps


def _pack(length):
    """The episodes, each put into the first sequence that still has room for it (at most ``length`` operations); a plain step goes in
    front of an episode that needs the z_mid its predecessor left unspecified."""
    seqs = []      # [operations, Shadow]
    for ep in _episodes():
        for cur, sh in seqs:
            ops, trial = list(ep), Shadow()
            trial.stale = sh.stale
            if not all(trial.legal(op) and (trial.take(op) or True) for op in ops):
                ops = [step(wait=False)] + ops
            if len(cur) + len(ops) <= length:
                break
        else:
            cur, sh, ops = [], Shadow(), list(ep)
            seqs.append((cur, sh))
        assert len(cur) + len(ops) <= length, (len(ops), length)
        for op in ops:
            assert sh.legal(op), (op, cur)
            sh.take(op)
        cur += ops
    return [cur for cur, _ in seqs]


_PACKED = {}


def planned(length=LENGTH):
    if length not in _PACKED:
        _PACKED[length] = _pack(length)
    return _PACKED[length]


def make_sequence(seed, length=LENGTH):
    """Sequence ``seed``: the planned episodes first (``len(planned(length))`` sequences fill REQUIRED); beyond them, episodes drawn at
    random: a situation, then a call into it.  About every second operation is a step."""
    plan = planned(length)
    if 0 <= seed < len(plan):
        return [(n, dict(a)) for n, a in plan[seed]]
    rng = Picker([7, seed])
    rng.turn = {k: rng.integers(12) for k in READERS + CHANGERS + ("ahead",)}
    seq, sh = [], Shadow()
    while len(seq) < length:
        sit = SINGLE[rng.integers(len(SINGLE))]
        kind = (READERS + CHANGERS)[rng.integers(len(READERS + CHANGERS))]
        ops = _setup(sit, rng, kind) + [_target(kind, rng, (sit,))]
        if rng.integers(3) == 0:      # one situation on top of another
            ops = _setup(SINGLE[rng.integers(len(SINGLE))], rng, "kkt") + ops
        trial = Shadow()
        trial.stale = sh.stale
        if not all(trial.legal(op) and (trial.take(op) or True) for op in ops):
            ops = [step(wait=False)] + ops
        for op in ops[:length - len(seq)]:
            if sh.legal(op):
                sh.take(op)
                seq.append(op)
    return seq


SEEDS = tuple(range(len(planned(LENGTH))))


# ---- the players' calls ----------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


def particles(tri, seed, count=PARTICLES):
    """``count`` starts: a vertex start and interior points, chosen by ``seed``."""
    rng = np.random.default_rng(seed)
    vt, vw = flow.vertex_starts(tri, int(tri.max()) + 1)
    v = int(rng.integers(vt.shape[0]))
    x = 0.05 + rng.random((count - 1, 3))
    t = np.concatenate([[vt[v]], rng.integers(0, tri.shape[0], count - 1)]).astype(np.int32)
    return t, np.ascontiguousarray(np.concatenate([vw[v][None], x / x.sum(axis=1, keepdims=True)]))


def host_decision(r, vals):
    """The factor the driver hands to adjust_penalty from conditions 0-3 as read (solver_socp.py: the penalty update), or None."""
    if vals is None or not set(vals) >= {0, 1, 2, 3}:
        return None
    policy = AdjustAdmmParam()
    if all(vals[i][0] < POLICY["tol"] for i in range(4)):
        return None
    prim, dual = max(vals[0][0], vals[1][0]), max(vals[2][0], vals[3][0])
    return policy.get_updated_value(r, prim / dual) / r


class Replay:
    """What the operations of one replay share: the model (the oracle ``s``: parameters and, loaded before every operation, the
    state), the mesh, the state ``before`` the operation on ``eager`` and the last conditions 0-3 ``lazy`` read."""

    def __init__(self, s, eager):
        self.s, self.tri = s, np.asarray(s.tri)
        self.nbr = flow.triangle_neighbours(self.tri)
        self.mu0, self.mu1 = -s.bnd[0] * (s.r * s.h), s.bnd[-1] * (s.r * s.h)      # (the end masses the players were created with)
        self.before, self.last_kkt = None, None
        self.model = sc.OracleDevice.__new__(sc.OracleDevice)      # the stand-in's formulas on the model's state
        self.model.s, self.model.strict, self.model.norm_d0 = s, False, math.sqrt(2.0 * s.area_mesh)
        self.model.palm = self.model.skip = self.model.stale = False
        if hasattr(eager, "plan"):
            import flow_checks
            import slide_checks

            self.tables = (slide_checks.caller_areas(eager.plan), flow_checks.caller_hat(eager.plan))
        else:
            self.tables = eager.flow_tables()

    def resolve(self, op):
        """The arguments both players get, formed once from the model: arrays from ``eager``'s state, scalars from the oracle's."""
        name, a = op
        s, out = self.s, dict(a)
        if name == "upload":
            out["x"] = self.before[a["name"]] * 1.01
        elif name == "adjust_penalty":
            f = a["f"]
            if a["how"] in ("confirm", "drop"):
                f = host_decision(s.r, self.last_kkt) or f
                f = f * DROP if a["how"] == "drop" else f
            out["f"], out["r"] = f, s.r * f
        elif name == "set_r":
            out["r"] = s.r * a["f"]
        elif name == "scale_z":
            out.update(sz=s.sz * a["f"], d=s.d * a["f"], norm_d=s.norm_d * a["f"])
        elif name == "apply_operator":
            out["x"] = self.before[OPERATORS[a["op"]]]
        elif name == "readout" and a["weighted"]:
            rng = np.random.default_rng(3)
            out["w_vertex"], out["w_triangle"] = rng.uniform(0.2, 2.0, s.V), rng.uniform(0.2, 2.0, s.F)
        elif name == "flow":
            out["tri"], out["w"] = particles(self.tri, a["seed"])
            out["span"] = (0, s.T) if a["call"] != "trace" else ((s.T, max(s.T - 2, 0)) if a["backward"] else (min(1, s.T - 1), min(3, s.T)))
            out["mass"] = np.linspace(0.5, 1.5, PARTICLES)
        elif name == "restart":
            out["mu0"], out["mu1"] = (self.mu1, self.mu0) if a["swap"] else (self.mu0, self.mu1)
        return out


def apply(dev, op, a, lazy):
    """The operation on a player; ``a``: its resolved arguments.  Returns what the call returns (None for a call that returns nothing)."""
    name = op[0]
    if name == "step":
        flags = a["flags"] if lazy else [f for f in a["flags"] if f == "palm"]
        dev.step_flags(**{f: True for f in flags})
        dev.step(1, wait=a["wait"])
    elif name == "kkt":
        return dev.kkt(a["mask"])
    elif name == "objective":
        return dev.objective()
    elif name == "norm_square":
        return dev.norm_square(a["name"], a["part"])
    elif name == "download":
        return dev.download(a["name"])
    elif name == "download_all":
        return dev.download_all()
    elif name == "upload":
        dev.upload(a["name"], a["x"])
    elif name == "adjust_penalty":
        dev.adjust_penalty(a["f"])
        dev.set_params(r=a["r"])
    elif name == "set_r":
        dev.set_params(r=a["r"])
    elif name == "scale_z":
        dev.scale_z(a["sz"], 1.0 / a["sz"], a["sz"])
        dev.set_params(scale_z=a["sz"], const_d=a["d"], norm_d=a["norm_d"])
    elif name == "scale_arrays":
        dev.scale_arrays(a["names"], a["f"])
    elif name == "run_phase":
        dev.run_phase(a["phase"])
    elif name == "apply_operator":
        return dev.apply_operator(a["op"], a["x"], 1.7)
    elif name == "readout":
        return dev.readout(a["factor"], a.get("w_vertex"), a.get("w_triangle"), a["centred"], a.get("mu0"), a.get("mu1"))
    elif name == "sensitivity":
        return dev.sensitivity(a["factor_phi"], a["factor_mu"], mass_vertex=a["mass_vertex"])
    elif name == "flow":
        args = (a["tri"], a["w"], a["nbr"], FLOOR)
        if a["call"] == "map":
            return dev.flow_map(*args, max_crossings=CROSSINGS)
        if a["call"] == "slide":
            return dev.flow_map(*args, max_crossings=CROSSINGS, slide=True)
        if a["call"] == "push":
            return dev.flow_push(*args, a["mass"], max_crossings=CROSSINGS)
        return dev.flow_trace(*args, a["span"], action=True, max_crossings=CROSSINGS)
    elif name == "restart":
        dev.restart(a["mu0"], a["mu1"], a["mode"], WARM_FACTORS if a["mode"] == "warm" else None)
    elif name == "penalty_ahead":
        if lazy:
            p = AdjustAdmmParam()
            dev.penalty_ahead(POLICY["tol"], POLICY["is_org_kkt"], p._sigma_lower_bound, p._sigma_upper_bound, p.FACTOR_STEPS)
    elif name == "refuse":
        what = a["what"]
        try:
            if what == "download_z_mid":
                dev.download("z_mid")
            elif what == "download_all":
                dev.download_all()
            elif what == "kkt_1":
                dev.kkt([1])
            elif what == "restart_warm":
                dev.restart(a["mu0"], a["mu1"], "warm", WARM_FACTORS)
            elif what == "palm_step":
                dev.step_flags(palm=True)
                dev.step(1, wait=False)
            elif what == "flags_palm_skip":
                dev.step_flags(palm=True, skip_z_mid=True)
            else:
                dev.step_flags(palm=True, rhs_ahead=True)
        except _lib.HipLibraryError as err:
            return ("refused", err.status)
        return ("refused", None)
    else:
        raise KeyError(name)
    return None


def same_result(name, x, y, fused=False):
    """``lazy``'s and ``eager``'s return values of one operation: the same bits; KKT values equal (within FUSED_TOL where the read may
    take the fused sums)."""
    if x is None or y is None:
        assert x is None and y is None, name
    elif isinstance(x, dict) and name == "kkt":
        assert x.keys() == y.keys(), name
        for i in x:
            for p, q in zip(x[i], y[i]):
                assert (p is None) == (q is None), (name, i)
                if p is not None and fused:
                    assert abs(p - q) <= FUSED_TOL * abs(q), (name, i, p, q)
                elif p is not None:
                    assert p == q, (name, i, p, q)
    elif isinstance(x, dict):
        assert x.keys() == y.keys(), (name, sorted(x), sorted(y))
        for k in x:
            same_result(f"{name}[{k}]", x[k], y[k])
    elif isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], str):
        assert x == y, (name, x, y)
    elif isinstance(x, (tuple, list)):
        assert len(x) == len(y), name
        for i, (p, q) in enumerate(zip(x, y)):
            same_result(f"{name}[{i}]", p, q)
    else:
        assert same(x, y), (name, "lazy and eager differ", np.asarray(x).shape)


def unchanged(before, after, but=()):
    for k in STATE:
        if k not in but:
            assert same(before[k], after[k]), (k, "changed")


def layer_sums_close(mu, mass, neg):
    """|sum - fsum| <= V 2^-52 sum |x| (test_hip_readout.check_sums)."""
    for l in range(mu.shape[0]):
        row = mu[l]
        bound = mu.shape[1] * 2.0 ** -52 * float(math.fsum(np.abs(row)))
        assert abs(mass[l] - math.fsum(row)) <= bound and abs(neg[l] - math.fsum(row[row < 0.0])) <= bound, l


NOISE = []      # (|got - want|, what the reordering moves) of every cancelling Dual(beta) read compared so far: what the docstrings record


def dual_beta_reordered(s):
    """What another order of summation moves in the oracle's kkt_dual_beta: the closure with the six terms of L^T beta_mid at a node -- three corners of the interval that starts there, three
    of the one that ends there -- added in another order: corner by corner from the last to the first, the ending interval first
    (the oracle adds the corners of each interval first, then the two intervals); returned is the residual of the DIFFERENCE of the two
    vectors E + L^T beta_mid, normalised as the closure normalises: by the triangle inequality no such reordering moves the value by
    more, while the difference of the two values themselves can be anything below it, by chance also next to nothing."""
    x = s.beta_mid
    p0, p1 = np.zeros((s.T + 1,) + x.shape[2:]), np.zeros((s.T + 1,) + x.shape[2:])      # (T + 1, 3, F, 3): zero where no interval is
    p0[:-1], p1[1:] = x[:, 0], x[:, 1]
    c = s.sz / O.SQRT3      # (... and every term scaled before it is added, the vertex part as sz beta_end - sz beta_fst)
    a2 = ((c * p1[:, 2] + c * p0[:, 2]) + (c * p1[:, 1] + c * p0[:, 1])) + (c * p1[:, 0] + c * p0[:, 0])
    a1 = s.sz * s.beta_end - s.sz * s.beta_fst
    nsum = s.r * (math.sqrt(s.nsq_time(s.mu) + s.nsq_space(s.E)) + math.sqrt(s.nsq_time(a1) + s.nsq_space(a2)))
    moved = s.r * math.sqrt(s.nsq_time((s.mu + a1) - (s.mu + s.sz * (s.beta_end - s.beta_fst)))
                            + s.nsq_space((s.E + a2) - (s.E + O.decouple_adjoint(x, s.sz))))
    return s._pair(moved, s.c_dual_beta, nsum, s.dual_scale)


def compare_kkt(s, state, got, conditions, cancelling=False):
    """``step_checks.compare_kkt``, as it stands, for every read but one kind.  ``cancelling`` (``cancelling_reads``): scale_z has SET
    mu and E to what makes Dual(beta) vanish, so that residual is rounding alone -- it depends on the order in which the six terms
    of L^T beta_mid are added, here and in the kernel that set E -- and no relative bound holds for it.  Its bound is measured on the
    oracle side, on the very state: what summing L^T beta_mid in another order moves in the oracle's own closure
    (``dual_beta_reordered``), times ``mode_checks.MARGIN``, on top of KKT_TOL |want|.  The other conditions of such a read keep the plain bound."""
    plain = [i for i in conditions if not (cancelling and i == 3)]
    sc.compare_kkt(s, state, got, conditions=plain)
    if len(plain) < len(list(conditions)):
        sc.load(s, state)
        want, moved = s.kkt_dual_beta(), dual_beta_reordered(s)
        for j in range(2):
            NOISE.append((abs(got[3][j] - want[j]), moved[j]))
            assert np.isfinite(want[j]) and abs(got[3][j] - want[j]) <= sc.KKT_TOL * abs(want[j]) + MARGIN * moved[j], \
                (3, j, got[3][j], want[j], moved[j])


def check_model(R, op, a, got, before, after):
    """``eager`` against the oracle: ``got`` is what the operation returned on it, ``after`` its state one operation after ``before``."""
    name, s = op[0], R.s
    sc.load(s, before)
    if name == "step":
        sc.check_one_step(s, before, after, palm="palm" in a["flags"])
    elif name == "kkt":
        unchanged(before, after)
        compare_kkt(s, before, got, a["mask"], cancelling=a["cancelling"])
    elif name == "objective":
        unchanged(before, after)
        for g, w in zip(got, s.objective()):
            assert abs(g - w) <= sc.FP_TOL * abs(w), ("objective", g, w)
    elif name == "norm_square":
        unchanged(before, after)
        want = R.model.norm_square(a["name"], a["part"])
        assert abs(got - want) <= NORM_TOL[(a["name"], a["part"])] * abs(want), ("norm_square", a, got, want)
    elif name == "download":
        unchanged(before, after)
        assert same(got, before[a["name"]]), a["name"]
    elif name == "download_all":
        unchanged(before, after)
        unchanged(before, got)
    elif name == "upload":
        unchanged(before, after, but=(a["name"],))
        assert same(after[a["name"]], a["x"]), a["name"]
    elif name == "adjust_penalty":
        want = sc.apply_penalty(s, before, a["f"])
        for k in STATE:
            sc.compare_entries(k, after[k], want[k])
    elif name == "set_r":
        unchanged(before, after)
        s.bnd *= s.r / a["r"]
        s.r = a["r"]
    elif name == "scale_z":
        s.scale_z(a["f"])
        s.sz, s.d, s.norm_d = a["sz"], a["d"], a["norm_d"]
        for k in STATE:
            sc.compare_entries(k, after[k], getattr(s, k))
    elif name == "scale_arrays":
        unchanged(before, after, but=a["names"])
        for k in set(a["names"]):
            sc.compare_entries(k, after[k], before[k] * a["f"])
    elif name == "run_phase":
        phase = a["phase"]
        if phase == "laplacian":
            unchanged(before, after, but=("phi",))
            s.step_laplacian()
            w = np.broadcast_to(s.mass_v[None, :], s.phi.shape)
            g, want = after["phi"] - np.sum(after["phi"] * w) / np.sum(w), s.phi - np.sum(s.phi * w) / np.sum(w)
            assert np.isfinite(g).all() and np.max(np.abs(g - want)) <= sc.PHI_TOL * np.max(np.abs(want)), "phi"
        else:
            {"soc_projection": s.step_soc_projection, "q_lambda": lambda: sc.palm_step0(s),
             "q_lambda_mult": lambda: (s.step_q_lambda(), s.step_multipliers())}[phase]()
            for k in STATE:
                sc.compare_entries(k, after[k], getattr(s, k))
    elif name == "apply_operator":
        unchanged(before, after)
        sc.compare_entries(a["op"], got, R.model.apply_operator(a["op"], a["x"], 1.7))
    elif name == "readout":
        unchanged(before, after)
        mu, E = readout.read_out_host({"mu": before["mu"], "E": before["E"]}, a["factor"], a.get("w_vertex"), a.get("w_triangle"), a["centred"],
                                      a.get("mu0"), a.get("mu1"))
        assert same(got[0], mu) and same(got[1], E), "readout"
        layer_sums_close(mu, got[2], got[3])
    elif name == "sensitivity":
        unchanged(before, after)
        phi0, phiT = sensitivity.potentials_host(before["phi"], a["factor_phi"])
        stress = sensitivity.stress_numpy(before["mu"], before["phi"], R.tri, a["mass_vertex"], a["factor_mu"], a["factor_phi"])
        assert same(got["phi0"], phi0) and same(got["phiT"], phiT) and same(got["stress"], stress), "sensitivity"
    elif name == "flow":
        unchanged(before, after)
        want = sc.trace_host(before["mu"], before["E"], R.tri, s.V, R.tables, a["tri"], a["w"], a["nbr"], FLOOR, a["span"],
                             action=a["call"] == "trace", mass=a["mass"] if a["call"] == "push" else None, max_crossings=CROSSINGS,
                             slide=a["call"] == "slide")
        same_result("flow " + a["call"], {k: got[k] for k in want}, want)
    elif name == "restart":
        R.model.restart(a["mu0"], a["mu1"], a["mode"], WARM_FACTORS)
        for k in STATE:
            assert same(after[k], getattr(s, k)), ("restart " + a["mode"], k)
    elif name == "refuse":
        unchanged(before, after)
    else:
        assert name == "penalty_ahead", name
        unchanged(before, after)


def replay(sequence, lazy, eager, oracle, on_step=None, report=None):
    """The sequence on the three players (module docstring).  ``lazy`` and ``eager`` hold the same state and the parameters of
    ``oracle`` (an OracleSolver) when the replay starts.  ``on_step(lazy)`` is called after every step on ``lazy`` (the step path);
    ``report`` (a list) takes one line per operation.  Raises AssertionError at the first difference."""
    assert legal(sequence), "the sequence breaks the caller's side of the rules"
    R = Replay(oracle, eager)
    sits, fused, cancelling = situations(sequence), fused_reads(sequence), cancelling_reads(sequence)
    state = eager.download_all()
    for i, op in enumerate(sequence):
        name = op[0]
        R.before = state
        a = R.resolve(op)
        a.update(nbr=R.nbr, mass_vertex=oracle.mass_v, cancelling=cancelling[i])
        if name in ("readout", "restart", "refuse"):
            a.setdefault("mu0", R.mu0), a.setdefault("mu1", R.mu1)
        where = (i, name, op[1], sorted(sits[i]))
        try:
            got_lazy = apply(lazy, op, a, True)
            if name == "step" and on_step is not None:
                on_step(lazy)
            both = name != "refuse" or REFUSALS[a["what"]][1]
            got_eager = apply(eager, op, a, False) if both else None
            after = eager.download_all()
            if name == "refuse":
                assert got_lazy == ("refused", REFUSALS[a["what"]][0]), ("lazy", got_lazy)
                assert not both or got_eager == got_lazy, ("eager", got_eager)
            else:
                same_result(name, got_lazy, got_eager, fused=fused[i])
            check_model(R, op, a, got_eager, state, after)
        except AssertionError as err:
            raise AssertionError(f"operation {where}: {err}") from err
        except _lib.HipLibraryError as err:
            # a status on a call the rules allow (a wrong DOTS_ERR_STATE, say) is a finding like any other; an error of the runtime
            # itself is not: it goes up as it is, and nothing is replayed on that device to shrink it
            if err.status in (ERR_ARGUMENT, ERR_STATE, _lib.ERR_MEMORY, -4):
                raise AssertionError(f"operation {where}: unexpected status {err.status}: {err}") from err
            raise
        if name == "kkt" and set(a["mask"]) >= {0, 1, 2, 3}:
            R.last_kkt = got_lazy
        if report is not None:
            report.append(where)
        state = after
    if stale_at_end(sequence):      # z_mid is unspecified on lazy: one more step on both stores it
        for dev in (lazy, eager):
            dev.step_flags()
            dev.step(1, wait=False)
    end_lazy, end_eager = lazy.download_all(), eager.download_all()
    for k in STATE:
        assert same(end_lazy[k], end_eager[k]), ("at the end", k, "lazy and eager differ")


def start(players, oracle, geom, seed):
    """Every player at the start of sequence ``seed``: the end masses and parameters of ``make_oracle``, the planted state
    ``edge_state(seed, zero_preimage=False)``; whatever the last sequence left pending is gone (a cold restart drops it)."""
    sc.edge_state(oracle, seed, zero_preimage=False)
    before = sc.snapshot(oracle)
    for dev in players:
        dev.restart(geom["mu0"], geom["mu1"], "cold")
        dev.step_flags()
        dev.set_params(**sc.device_params(oracle))
        for k in STATE:
            dev.upload(k, before[k])
    return before


def congestion_of(seed):
    return 0.05 if seed % 2 else 0.0


# ---- shrinking ---------------------------------------------------------------------------------------------------------------------------
def shrink(sequence, fails):
    """Greedy: drop single operations while ``fails(sequence)`` still holds and the caller's rules still do; the result fails and no
    single operation can be removed from it."""
    seq = list(sequence)
    assert fails(seq), "the sequence does not fail"
    again = True
    while again:
        again = False
        for i in range(len(seq)):
            cand = seq[:i] + seq[i + 1:]
            if legal(cand) and fails(cand):
                seq, again = cand, True
                break
    return seq


def fails_on(make_players):
    """The predicate of ``shrink``: ``make_players()`` -> ``(lazy, eager, oracle, geom, seed, close)`` on fresh players."""
    def fails(seq):
        lazy, eager, oracle, geom, seed, close = make_players()
        try:
            start((lazy, eager), oracle, geom, seed)
            replay(seq, lazy, eager, oracle)
        except AssertionError:
            return True
        finally:
            close()
        return False
    return fails


# ---- regressions -------------------------------------------------------------------------------------------------------------------------
# name -> (seed of the start state, the shrunk sequence): sequences that failed on the device once, replayed by both tests
REGRESSIONS = {}
