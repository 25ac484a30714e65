"""What the checks of the TIME-SLAB iteration share (test_hip_sharded.py, test_hip_slab_steps.py, test_slab_checks_cpu.py; plain numpy,
TEST INFRASTRUCTURE):

``SlabGroup``   n time-slab contexts driven from ONE thread, the exchanges plain copies; over ``DeviceProblem`` with torch CUDA buffers, or
                over ``fake_device.FakeDeviceProblem`` with numpy buffers;
``SlabDevice``  the calls the scenarios of step_checks.py make, played by a group: whole arrays in, whole arrays out;
``PARTITIONS``  the (T, ranks) cases with what each implies, as literals;
``slab_cells``  where a planted state puts its special columns on a partition: next to the slab boundaries."""
import numpy as np

import step_checks as sc

O = sc.O
BUFFERS = ("send_x", "send_nsq", "recv_x", "recv_nsq", "b_send", "b_recv", "x_send", "x_recv", "send_mu", "send_b", "recv_mu", "recv_b")
CORNER = ("z_mid", "beta_mid")

# (T, ranks) -> (nodes, intervals) per rank, slab time pitch; written out: a change of distributed.slab_partition fails this table first
PARTITIONS = {
    (1, 2): (((1, 1), (1, 0)), 4),                                                   # a rank with a node and no interval
    (5, 6): (((1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 0)), 4),                   # every column is a halo column
    (4, 8): (((1, 1), (1, 1), (1, 1), (1, 1), (1, 0), (0, 0), (0, 0), (0, 0)), 4),   # empty ranks inside the exchanges
    (6, 3): (((3, 3), (3, 3), (1, 0)), 4),                                           # the last rank holds node T only
    (8, 2): (((5, 5), (4, 3)), 8),                                                   # ragged pitch
    (31, 3): (((11, 11), (11, 11), (10, 9)), 16),                                    # ragged; odd and even slab lengths
    (31, 1): (((32, 31),), 32),                                                      # one rank through the slab stages
    (63, 2): (((32, 32), (32, 31)), 32),                                             # full pitch
    (64, 5): (((13, 13), (13, 13), (13, 13), (13, 13), (13, 12)), 16),               # odd T
    (127, 2): (((64, 64), (64, 63)), 64),
    (255, 2): (((128, 128), (128, 127)), 128),                                       # T + 1 = 256, the slab limit; the largest pitch that carries
    (255, 1): (((256, 255),), 256),                                                  # no carry possible (pitch above 128)
}
SMALL_PITCH, LARGE_PITCH = (6, 3), (127, 2)      # the two partitions of the scenarios that do not run on all of them
CARRY_MAX_PITCH = 128                             # csrc/dots_dev.h: carry_possible


# the seed of the planted state: T, as in test_hip_step_variants, wherever the conditions on the input hold with it (every branch on every
# interval next to a slab boundary, in all four variants the scenarios plant); the fan at T = 64 needs another one
SEEDS = {("fan", (64, 5)): 1000}


def seed_for(mesh, partition):
    return SEEDS.get((mesh, partition), partition[0])


def partition_id(p):
    return f"T{p[0]}x{p[1]}"


def first_nodes(partition):
    """The first node of every rank that holds one."""
    out, n0 = [], 0
    for nl, _ in PARTITIONS[partition][0]:
        if nl:
            out.append(n0)
        n0 += nl
    return out


def boundary_intervals(partition):
    """The intervals next to a slab boundary: the one that ends at a slab's first node and the one that starts there."""
    T = partition[0]
    out = []
    for n0 in first_nodes(partition)[1:]:
        out += [t for t in (n0 - 1, n0) if 0 <= t < T and t not in out]
    return out


def slab_cells(partition):
    """name -> interval for ``step_checks.edge_state``: one zero pre-image, one column on the upper and one on the lower boundary of the
    cone at the LAST interval of the first slab (its cone norm is half recv_nsq, its multiplier travels in the tail of x_send), at the
    FIRST interval of the second slab, and -- where a rank holds a single node -- at the interval that ends at the last such node."""
    T = partition[0]
    starts = first_nodes(partition)
    if len(starts) == 1:
        return None                               # one rank: no boundary; the default places
    at = [starts[1] - 1] + ([starts[1]] if starts[1] < T else [])
    n0 = 0
    for nl, _ in PARTITIONS[partition][0]:
        if nl == 1 and n0 > 0 and n0 - 1 not in at:
            at = at[:2] + [n0 - 1]                # (the last one wins: three places at the most)
        n0 += nl
    if len(at) == 1:
        at = at * 2                               # T = 1: everything sits on the one interval, as with the default places
    return {f"{kind}{i}": t for i, t in enumerate(at) for kind in ("nan", "up", "lo")}


def make_oracle(T, geom, congestion=0.0, eps=0.0):
    """step_checks.make_oracle, with the regularisation of the solve."""
    s = O.OracleSolver(T, geom, congestion=congestion, eps=eps)
    s.r, s.sz, s.d = 1.7, 2.5, 1.3
    s.norm_d *= 1.3
    s.bnd /= s.r
    return s


# ---- exchange buffers -----------------------------------------------------------------------------------------------------------
class TorchBuffers:
    """float64 CUDA tensors."""

    def __init__(self):
        import torch

        self.torch = torch

    def zeros(self, n):
        return self.torch.zeros(n, dtype=self.torch.float64, device="cuda")

    @staticmethod
    def ptr(t):
        return t.data_ptr()

    @staticmethod
    def copy(dst, src):
        dst.copy_(src)

    def cat(self, parts):
        return self.torch.cat(parts)

    def sync(self):
        self.torch.cuda.synchronize()


class NumpyBuffers:
    """float64 host arrays (the CPU stand-in reads and writes them through their addresses)."""

    @staticmethod
    def zeros(n):
        return np.zeros(n)

    @staticmethod
    def ptr(a):
        return a.ctypes.data

    @staticmethod
    def copy(dst, src):
        dst[:] = src

    @staticmethod
    def cat(parts):
        return np.concatenate(parts)

    @staticmethod
    def sync():
        pass


class SlabGroup:
    """n time-slab contexts driven from ONE thread of one process: the exchanges are plain copies.  ``rank_class``: ``DeviceProblem``
    (default) or ``fake_device.FakeDeviceProblem``; ``buffers``: ``TorchBuffers()`` (default) or ``NumpyBuffers()``.  ``defer_buffers``: the
    ranks get their exchange buffers only with ``set_buffers()`` (after a factor was installed, say), not here."""

    def __init__(self, T, geom, n_ranks, rank_class=None, buffers=None, defer_buffers=False, **kw):
        if rank_class is None:
            from dots_socp_amd.device import DeviceProblem as rank_class
        self.buffers = buffers if buffers is not None else TorchBuffers()
        self.n = n_ranks
        self.devs = [rank_class(T, geom, lap_solver="modal_pcg", time_slab=(r, n_ranks), **kw) for r in range(n_ranks)]
        self.bufs = []
        z = self.buffers.zeros
        for d in self.devs:
            nv, nf, nb, nx = (d.slab_elems(k) for k in ("vertex_halo", "triangle_halo", "b_chunk", "x_chunk"))
            b = {"send_x": z(nv), "send_nsq": z(nv), "recv_x": z(nv), "recv_nsq": z(nv), "b_send": z(nb), "b_recv": z(nb * n_ranks),
                 "x_send": z(nx), "x_recv": z(nx * n_ranks), "send_mu": z(nv), "send_b": z(nf), "recv_mu": z(nv), "recv_b": z(nf)}
            self.bufs.append(b)
        if not defer_buffers:
            self.set_buffers()
        self.active = self.devs[0].active_ranks

    def set_buffers(self):
        for d, b in zip(self.devs, self.bufs):
            d.slab_set_buffers(**{k: self.buffers.ptr(t) for k, t in b.items()})

    def each(self, fn):
        return [fn(d) for d in self.devs]

    def upload(self, state):
        for d in self.devs:
            if d.nl:
                for k, v in state.items():
                    d.upload(k, d.to_slab(k, v, with_next_node=k == "phi"))

    def neighbours(self, fwd, bwd):
        for d in self.devs:
            d.sync()
        for r in range(self.active):
            if r > 0:
                self.buffers.copy(self.bufs[r][fwd[1]], self.bufs[r - 1][fwd[0]])
            if r + 1 < self.active:
                self.buffers.copy(self.bufs[r][bwd[1]], self.bufs[r + 1][bwd[0]])
        self.buffers.sync()

    def gather(self, send, recv):
        for d in self.devs:
            d.sync()
        allv = self.buffers.cat([b[send] for b in self.bufs])
        for b in self.bufs:
            self.buffers.copy(b[recv], allv)
        self.buffers.sync()

    def iterate(self, split=None, wait=False):
        """``split``: stage 1 in its two halves (6: right-hand side, 5: projection) around the all-gather of b; default: every other iteration."""
        import pytest

        self.n_iterations = getattr(self, "n_iterations", 0) + 1
        if split is None:
            split = self.n_iterations % 2 == 0
        self.each(lambda d: d.slab_stage(0, wait=wait))
        self.neighbours(("send_x", "recv_x"), ("send_nsq", "recv_nsq"))
        if split:
            self.each(lambda d: d.slab_stage(6, wait=wait))
            self.gather("b_send", "b_recv")
            self.each(lambda d: d.slab_stage(5, wait=wait))
            with pytest.raises(Exception, match="order"):
                self.devs[0].slab_stage(5)
        else:
            self.each(lambda d: d.slab_stage(1, wait=wait))
            self.gather("b_send", "b_recv")
        self.each(lambda d: d.slab_stage(2, wait=wait))
        self.gather("x_send", "x_recv")
        self.each(lambda d: d.slab_stage(3, wait=wait))

    def kkt(self, conditions):
        self.each(lambda d: d.slab_stage(4))
        self.neighbours(("send_mu", "recv_mu"), ("send_b", "recv_b"))
        total = sum(d.kkt_sums(conditions) for d in self.devs)
        return self.devs[0].kkt_combine(conditions, total)

    def objective(self):
        return self.devs[0].objective_combine(sum(d.objective_sums() for d in self.devs))

    def download(self, name):
        full = np.zeros(self.devs[0].full_shape(name))
        for d in self.devs:
            if d.nl:
                d.from_slab(name, d.download(name), full)
        return full

    def close(self):
        self.each(lambda d: d.close())


class SlabDevice:
    """The calls the scenarios of step_checks make (``DeviceProblem``'s, on whole arrays), played by a ``SlabGroup``.
    ``split``: the stage order 0, 6, 5, 2, 3 instead of 0, 1, 2, 3.  ``cells`` / ``boundary``: read by step_checks._upload.
    ``nan_slots``: the slots of a slab's corner arrays whose interval does not exist are NaN on upload (they are to be ignored).
    ``defect``: a deliberate defect of the upload -- "to_slab_shift": the s = 1 half of a corner array lands one node late;
    "phi_without_next_node": phi comes without the next slab's first node (the slab then keeps what its last solve left there)."""

    def __init__(self, group, partition=None, split=False, nan_slots=False, defect=None):
        self.group, self.split, self.nan_slots, self.defect = group, split, nan_slots, defect
        self.cells = slab_cells(partition) if partition is not None else None
        self.boundary = boundary_intervals(partition) if partition is not None else ()

    def slab_part(self, d, name, whole):
        part = d.to_slab(name, whole, with_next_node=name == "phi" and self.defect != "phi_without_next_node")
        if name in CORNER:
            if self.defect == "to_slab_shift":
                part[:, 1] = np.roll(part[:, 1], 1, axis=0)
            if self.nan_slots:
                if d.node0 == 0:
                    part[0, 1] = np.nan           # interval -1
                if d.ni < d.nl:
                    part[d.ni:, 0] = np.nan       # interval T
        return part

    def upload(self, name, whole):
        for d in self.group.devs:
            if d.nl:
                d.upload(name, self.slab_part(d, name, np.asarray(whole, dtype=np.float64)))

    def download(self, name):
        return self.group.download(name)

    def download_all(self):
        return {k: self.download(k) for k in sc.STATE}

    def set_params(self, **kw):
        self.group.each(lambda d: d.set_params(**kw))

    def adjust_penalty(self, factor):
        self.group.each(lambda d: d.adjust_penalty(factor))

    def step_flags(self, **kw):
        self.group.each(lambda d: d.step_flags(**kw))

    def step(self, n=1, wait=True):
        for _ in range(n):
            self.group.iterate(split=self.split, wait=wait)

    def kkt(self, conditions):
        return self.group.kkt(list(conditions))

    def objective(self):
        return self.group.objective()

    def debug_counter(self, which=0):
        """Per rank."""
        return [d.debug_counter(which) for d in self.group.devs]

    def close(self):
        self.group.close()


# ---- the checks both sides run (the GPU's contexts, or the CPU stand-in) ---------------------------------------------------------------
def run_scenario(group, name, s, partition, seed, split=False, expect=None):
    """A scenario of step_checks on a group whose ranks are set up (factor installed, cg_tol set) and hold no state yet."""
    dev = SlabDevice(group, partition, split=split)
    dev.set_params(**sc.device_params(s))
    sc.scenario(name)(dev, s, partition[0], seed=seed, expect=expect or (lambda *a, **k: None))
    return dev


def plant(dev, s, seed):
    """A planted state without a zero pre-image (nothing after it is NaN) on the oracle and on the slabs."""
    dev.set_params(**sc.device_params(s))
    before, masks = sc._upload(dev, s, seed, zero_preimage=False)
    sc.assert_edge_properties(masks, zero_preimage=False)
    return before


def check_kkt_and_objective(group, s, partition, seed):
    """One step, then all seven residuals through the slabs' sums (conditions 2 and 5 read mu_lo, condition 4 reads B_hi across the slab
    boundary) and the objective, against the oracle on the state the slabs hold."""
    dev = SlabDevice(group, partition)
    before = plant(dev, s, seed)
    dev.step_flags()
    dev.step(1, wait=False)
    after = dev.download_all()
    figures = sc.check_one_step(s, before, after)
    sc.compare_kkt(s, after, dev.kkt(range(7)), conditions=range(7))      # (leaves the oracle holding ``after``)
    got, want = dev.objective(), s.objective()
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), (got, want)                  # (test_hip_phases: test_kkt_objective_norms_a10_a11_a12)
    return figures


def check_stage_orders(group_a, group_b, s, partition, seed):
    """Stages 0, 1, 2, 3 and 0, 6, 5, 2, 3 from the same planted state: all twelve arrays bit for bit the same."""
    out = []
    for group, split in ((group_a, False), (group_b, True)):
        dev = SlabDevice(group, partition, split=split)
        plant(dev, s, seed)
        dev.step_flags()
        dev.step(1, wait=False)
        out.append(dev.download_all())
    for k in sc.STATE:
        assert np.array_equal(out[0][k], out[1][k]), k


def check_layout(group_a, group_b, s, partition, seed):
    """Upload and download return the twelve planted arrays bit for bit; NaN in the slots of a slab's corner arrays whose interval does not
    exist reaches no download and no step result."""
    plain, with_nan = SlabDevice(group_a, partition), SlabDevice(group_b, partition, nan_slots=True)
    before = plant(plain, s, seed)
    plant(with_nan, s, seed)
    for dev in (plain, with_nan):
        back = dev.download_all()
        for k in sc.STATE:
            assert np.array_equal(back[k], before[k]), k
    out = []
    for dev in (plain, with_nan):
        dev.step_flags()
        dev.step(1, wait=False)
        out.append(dev.download_all())
    for k in sc.STATE:
        assert np.isfinite(out[1][k]).all(), k
        assert np.array_equal(out[0][k], out[1][k]), k
