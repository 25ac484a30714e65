"""DeviceProblem: one device-resident DOTs-SOCP problem behind the C ABI.

Thin object wrapper over ``libdotsocp_hip.so``: builds the problem description from the host-side
plan (``geometry.build_plan``), owns the context handle, and exposes the calls of
``include/dots_socp_hip.h`` with numpy arrays in the reference's layouts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .geometry import DevicePlan, build_plan

STATE_NAMES = tuple(_lib.ARRAY_IDS)


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def place_slab(name, part, full, n0, nl, ni):
    """Write the part of the slab that holds the nodes ``[n0, n0 + nl)`` (``ni`` intervals) into a whole array in the reference
    layout; ``part`` may be longer than the slab along its first axis (padding is ignored).  Corner arrays are indexed by the
    node an entry is compared with (include/dots_socp_hip.h)."""
    if name in ("z_mid", "beta_mid"):
        full[n0:n0 + ni, 0] = part[:ni, 0]
        lo = 1 if n0 == 0 else 0                           # entry [j][1] is the reference's [n0 + j - 1][1]
        full[n0 + lo - 1:n0 + nl - 1, 1] = part[lo:nl, 1]
    else:
        n = nl if name in ("phi", "B", "E") else ni
        full[n0:n0 + n] = part[:n]
    return full


PCG_WINDOW = 256          # time modes per window of the windowed modal PCG (dots_pcg_windows)
MAX_TIME_NODES = 1024     # T + 1 one context takes


def pcg_window_plan(n_time):
    """``[(first_mode, live_columns), ...]``: the windows of 256 time modes the windowed modal PCG (dots_pcg_windows) solves one after
    the other at ``n_time + 1`` nodes.  Up to 256 nodes that is the one window the PCG always had; a window without a live mode
    (the fourth at 600 intervals, pitch 1024) is not listed: it is neither written nor solved."""
    nodes = int(n_time) + 1
    if nodes < 2 or nodes > MAX_TIME_NODES:
        raise ValueError(f"pcg_window_plan: n_time + 1 = {nodes} time nodes, the library takes 2 to {MAX_TIME_NODES}")
    return [(first, min(PCG_WINDOW, nodes - first)) for first in range(0, nodes, PCG_WINDOW)]


class DeviceProblem:
    def __init__(self, n_time, geometry, lap_solver="spacetime_pcg", device=0, reorder=True, plan: DevicePlan | None = None,
                 time_slab=None, nd_leaf=16, pcg_windows=False):
        """``time_slab = (rank, n_ranks)``: this context is one TIME SLAB of a multi-GPU solve (distributed.py): it holds
        the nodes [rank * stride, ...) of every state array and solves the time modes with the same indices; the caller
        drives ``slab_stage`` around its exchanges.  ``pcg_windows``: ``enable_pcg_windows()`` right after creation."""
        self.lib = _lib.load()
        self.plan = plan if plan is not None else build_plan(n_time, geometry, reorder=reorder, nd_leaf=nd_leaf)
        p = self.plan
        self.T, self.V, self.F = p.n_time, p.n_vertices, p.n_triangles
        if lap_solver not in _lib.LAP_SOLVERS:
            raise ValueError(f"lap_solver must be one of {list(_lib.LAP_SOLVERS)}")
        self.lap_solver = lap_solver
        d = _lib.ProblemDesc()
        d.abi_version = _lib.ABI_VERSION
        d.device = self.device = int(device)
        d.n_time, d.n_vertices, d.n_triangles = p.n_time, p.n_vertices, p.n_triangles
        d.n_corners = int(p.corner_idx.size)
        d.lap_nnz = int(p.lap_val.size)
        d.lap_solver = _lib.LAP_SOLVERS[lap_solver]
        d.triangles = _ptr(p.triangles, C.c_int32)
        d.hat_grad = _ptr(p.hat_grad, C.c_double)
        d.area_tri = _ptr(p.area_tri, C.c_double)
        d.mass_vert = _ptr(p.mass_vert, C.c_double)
        d.corner_ptr = _ptr(p.corner_ptr, C.c_int32)
        d.corner_idx = _ptr(p.corner_idx, C.c_int32)
        d.lap_rowptr = _ptr(p.lap_rowptr, C.c_int32)
        d.lap_col = _ptr(p.lap_col, C.c_int32)
        d.lap_val = _ptr(p.lap_val, C.c_double)
        d.mu0 = _ptr(p.mu0, C.c_double)
        d.mu1 = _ptr(p.mu1, C.c_double)
        d.perm_vert = _ptr(p.perm_vert, C.c_int32)
        d.perm_tri = _ptr(p.perm_tri, C.c_int32)
        d.time_modes = _ptr(p.time_modes, C.c_double)
        d.time_eigs = _ptr(p.time_eigs, C.c_double)
        self.mode_slice = None
        self.node0, self.nl, self.ni = 0, p.n_time + 1, p.n_time
        self.slab = None
        if time_slab is not None:
            rank, n_ranks = time_slab
            stride = -(-(p.n_time + 1) // n_ranks)
            begin = min(rank * stride, p.n_time + 1)
            count = max(0, min(stride, p.n_time + 1 - begin))
            d.slab_begin, d.slab_count, d.slab_stride = (begin if count else 0), count, stride
            self.mode_slice = slice(begin, begin + count)       # modes solved here = nodes held here
            self.slab = (rank, n_ranks, stride)
            self.node0, self.nl, self.ni = begin, count, max(0, min(count, p.n_time - begin))
            self.active_ranks = -(-(p.n_time + 1) // stride)    # ranks that hold at least one node
        self._h = C.c_void_p()
        _lib.check(self.lib.dots_create(C.byref(d), C.byref(self._h)), "dots_create")
        self.params = _lib.Params()
        _lib.check(self.lib.dots_get_params(self._h, C.byref(self.params)), "dots_get_params")
        self.pcg_windows = False
        if pcg_windows:
            try:
                self.enable_pcg_windows()
            except Exception:
                self.close()
                raise

    # ---- lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.dots_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- shapes of the host arrays: the reference layouts on one GPU, the slab's time extent on a time slab
    def shape(self, name):
        V, F = self.V, self.F
        if name == "phi":
            return (self.nl, V)
        if name in ("B", "E"):
            return (self.nl, F, 3)
        if name in ("z_mid", "beta_mid"):
            return ((self.nl if self.slab else self.ni), 2, 3, F, 3)
        return (self.ni, V)

    def full_shape(self, name):
        T, V, F = self.T, self.V, self.F
        return {"phi": (T + 1, V), "B": (T + 1, F, 3), "E": (T + 1, F, 3), "z_mid": (T, 2, 3, F, 3), "beta_mid": (T, 2, 3, F, 3)}.get(name, (T, V))

    def to_slab(self, name, full, with_next_node=False):
        """This slab's part of a whole array in the reference layout, of shape ``shape(name)`` (see include/dots_socp_hip.h: the
        corner arrays are indexed by the node an entry is compared with).  ``with_next_node``: phi with the next slab's first
        node as one more row, where a next slab exists -- the form in which ``upload`` also sets that node."""
        full = np.asarray(full, dtype=np.float64)
        n0, nl, ni = self.node0, self.nl, self.ni
        if name in ("z_mid", "beta_mid"):
            out = np.zeros(self.shape(name))
            out[:ni, 0] = full[n0:n0 + ni, 0]
            lo = 1 if n0 == 0 else 0                           # entry [j][1] is the reference's [n0 + j - 1][1]
            out[lo:nl, 1] = full[n0 + lo - 1:n0 + nl - 1, 1]
            return out
        if with_next_node and name == "phi" and self.slab and nl and n0 + nl <= self.T:
            return np.ascontiguousarray(full[n0:n0 + nl + 1])      # ... and the next slab's first node (``upload``)
        return np.ascontiguousarray(full[n0:n0 + (nl if name in ("phi", "B", "E") else ni)])

    def from_slab(self, name, part, full):
        """Write this slab's part into a whole array in the reference layout (entries of other slabs untouched)."""
        return place_slab(name, part, full, self.node0, self.nl, self.ni)

    # ---- parameters
    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(k)
            setattr(self.params, k, v)
        _lib.check(self.lib.dots_set_params(self._h, C.byref(self.params)), "dots_set_params")

    # ---- state transfer
    def upload(self, name, array):
        a = np.ascontiguousarray(array, dtype=np.float64)
        # a time slab's phi may come with the next slab's first node as one more row (``to_slab(..., with_next_node=True)``): only this rank's
        # solves write that node otherwise, and step 0 of is_palm and the KKT residuals read it
        with_next = name == "phi" and self.slab and self.nl and self.node0 + self.nl <= self.T and a.shape == (self.nl + 1, self.V)
        if a.shape != self.shape(name) and not with_next:
            raise ValueError(f"{name}: expected shape {self.shape(name)}, got {a.shape}")
        _lib.check(self.lib.dots_upload(self._h, _lib.ARRAY_IDS[name], _ptr(a, C.c_double), a.size), f"upload {name}")

    def download(self, name):
        out = np.empty(self.shape(name), dtype=np.float64)
        _lib.check(self.lib.dots_download(self._h, _lib.ARRAY_IDS[name], _ptr(out, C.c_double), out.size), f"download {name}")
        return out

    def download_all(self):
        return {n: self.download(n) for n in STATE_NAMES}

    def readout(self, factor=1.0, w_vertex=None, w_triangle=None, centred=False, mu0=None, mu1=None, mu=True, E=True, sums=True):
        """``(mu, E, layer_mass, layer_negative)`` formed on the device (dots_readout; readout.read_out_host is the specification):
        ``mu`` (T, V) -- (T + 1, V) when ``centred`` -- and ``E`` (T + 1, F, 3), every value times ``factor``, then times its
        vertex's / triangle's weight where given; the sum of every layer of ``mu`` and of its negative entries.  ``mu`` / ``E`` /
        ``sums`` = False leave that part out (None).  ``self.readout_ms`` / ``self.readout_bytes``: device milliseconds of the
        launches and the bytes copied to the host by the last call."""
        if self.slab:
            raise ValueError("readout: not available on time slabs")
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
        wv, wt, m0, m1 = f64(w_vertex), f64(w_triangle), f64(mu0), f64(mu1)
        for a, n, what in ((wv, self.V, "w_vertex"), (m0, self.V, "mu0"), (m1, self.V, "mu1"), (wt, self.F, "w_triangle")):
            if a is not None and a.shape != (n,):
                raise ValueError(f"readout: {what} must have shape ({n},), got {a.shape}")
        layers = self.T + (1 if centred else 0)
        out_mu = np.empty((layers, self.V)) if mu else None
        out_E = np.empty((self.T + 1, self.F, 3)) if E else None
        mass, neg = (np.empty(layers), np.empty(layers)) if sums else (None, None)
        ms = C.c_double()
        d = _lib.ReadoutDesc()
        d.factor, d.centred = float(factor), int(bool(centred))
        d.w_vertex, d.w_triangle, d.mu0, d.mu1 = _ptr(wv, C.c_double), _ptr(wt, C.c_double), _ptr(m0, C.c_double), _ptr(m1, C.c_double)
        d.mu, d.E, d.layer_mass, d.layer_negative = _ptr(out_mu, C.c_double), _ptr(out_E, C.c_double), _ptr(mass, C.c_double), _ptr(neg, C.c_double)
        d.ms = C.pointer(ms)
        before = self.debug_counter(9)
        _lib.check(self.lib.dots_readout(self._h, C.byref(d)), "dots_readout")
        self.readout_ms, self.readout_bytes = ms.value, self.debug_counter(9) - before
        return out_mu, out_E, mass, neg

    def sensitivity(self, factor_phi=1.0, factor_mu=1.0, mass_vertex=None, potentials=True, stress=True, to_device=False):
        """``{"phi0", "phiT", "stress"}`` formed on the device (dots_sensitivity; sensitivity.potentials_host and stress_host on the
        downloaded ``phi`` and ``mu`` are the specification and return the same bits): ``phi0`` / ``phiT`` (V,) the potential at the two
        ends times ``factor_phi``, ``stress`` (F, 3, 6) of ``factor_mu * mu``, ``factor_phi * phi`` and the vertex masses
        ``mass_vertex`` (V,) in the caller's numbering (None: the context's own).  ``potentials`` / ``stress`` = False leave that part
        out.  ``to_device``: torch tensors on the context's device, written by the kernels themselves -- nothing crosses to the host.
        ``self.sensitivity_ms`` / ``self.sensitivity_bytes``: device milliseconds of the launches and bytes copied to the host."""
        if self.slab:
            raise ValueError("sensitivity: not available on time slabs")
        if not potentials and not stress:
            raise ValueError("sensitivity: nothing asked for (potentials and stress are both False)")
        mass = None if mass_vertex is None else np.ascontiguousarray(mass_vertex, dtype=np.float64)
        if mass is not None and mass.shape != (self.V,):
            raise ValueError(f"sensitivity: mass_vertex must have shape ({self.V},), got {mass.shape}")
        shapes = {}
        if potentials:
            shapes["phi0"] = shapes["phiT"] = (self.V,)
        if stress:
            shapes["stress"] = (self.F, 3, 6)
        if to_device:
            import torch

            where = torch.device("cuda", self.device)
            out = {k: torch.empty(s, dtype=torch.float64, device=where) for k, s in shapes.items()}
            torch.cuda.current_stream(where).synchronize()      # (the kernels write on the context's stream: nothing of torch's is pending on the memory)
            address = {k: a.data_ptr() for k, a in out.items()}
        else:
            out = {k: np.empty(s) for k, s in shapes.items()}
            address = {k: a.ctypes.data for k, a in out.items()}
        ms = C.c_double()
        d = _lib.SensitivityDesc()
        d.factor_phi, d.factor_mu, d.mass_vertex = float(factor_phi), float(factor_mu), _ptr(mass, C.c_double)
        d.phi0, d.phiT, d.stress = address.get("phi0"), address.get("phiT"), address.get("stress")
        d.device_pointers = int(bool(to_device))
        d.ms = C.pointer(ms)
        before = self.debug_counter(9)
        _lib.check(self.lib.dots_sensitivity(self._h, C.byref(d)), "dots_sensitivity")
        self.sensitivity_ms, self.sensitivity_bytes = ms.value, self.debug_counter(9) - before
        return out

    def flow_map(self, start_triangle, start_weights, neighbours, floor, max_crossings=16, trajectory=False, slide=False):
        """Trace particles through the transport the context holds, on the device (dots_flow_map; flow.flow_map_host on the downloaded
        ``mu`` and ``E`` is the specification and returns the same bits).  ``start_triangle`` (P,), ``start_weights`` (P, 3) and
        ``neighbours`` (F, 3) (``flow.triangle_neighbours``) in the caller's numbering; ``floor`` in the units of the iterate as stored.
        Returns the dict of ``flow_map_host``.  ``self.flow_map_ms`` / ``self.flow_map_bytes``: device milliseconds of the launch and
        the bytes copied to the host by the last call.  ``slide``: the sliding mode on edges where two triangles push a particle at
        each other (dots_flow_slide; ``flow_map_host(..., slide=True, areas=plan.area_tri)`` is the specification): the call is
        ``flow_trace`` over ``(0, n_time)`` with ``slide=True``, and the result gains ``"slides"`` and ``"steps"``."""
        if self.slab:
            raise ValueError("flow_map: not available on time slabs")
        if slide:
            out = self.flow_trace(start_triangle, start_weights, neighbours, floor, (0, self.T), max_crossings=max_crossings, trajectory=trajectory,
                                  slide=True)
            self.flow_map_ms, self.flow_map_bytes = self.flow_trace_ms, self.flow_trace_bytes
            return out
        return self._flow("flow_map", start_triangle, start_weights, neighbours, floor, max_crossings, trajectory)

    def flow_push(self, start_triangle, start_weights, neighbours, floor, mass, attributes=None, exponents=None, layers="end",
                  max_crossings=16, trajectory=False):
        """``flow_map`` and, summed onto the vertices on the device, what the particles carry (dots_flow_push; flow.push_forward_host
        on the result of ``flow_map(..., trajectory=True)`` is the specification and returns the same bits): ``mass`` (P,),
        ``attributes`` None or (A <= 4, P), ``exponents`` (1 + A,) (default ``flow.push_scales``), ``layers`` "end" or "all".
        Returns the dict of ``flow_map`` plus ``"mass_at"`` (L, V), ``"attr_at"`` (A, L, V) or None, ``"dropped"`` and ``"exponents"``.
        ``self.flow_push_ms`` / ``self.flow_push_bytes``: device milliseconds (zeroing, trace with deposits, conversion) and the
        bytes copied to the host by the last call."""
        return self._flow("flow_push", start_triangle, start_weights, neighbours, floor, max_crossings, trajectory, mass=mass, attributes=attributes,
                          exponents=exponents, layers=layers)

    def flow_trace(self, start_triangle, start_weights, neighbours, floor, span, action=False, mass=None, attributes=None, exponents=None,
                   layers="end", max_crossings=16, trajectory=False, slide=False):
        """``flow_map`` between the time nodes ``span = (node_from, node_to)``, backward where ``node_to < node_from`` (dots_flow_trace;
        ``flow.flow_map_host(..., span=span, action=action)`` on the downloaded ``mu`` and ``E`` is the specification and returns the
        same bits).  ``action``: the result gains ``"action"`` (P,).  ``mass`` (P,): also the deposits of ``flow_push`` on the layers of
        this trace (``attributes``, ``exponents``, ``layers`` as there; ``"end"`` is the state at ``node_to``), and the result gains what
        ``flow_push`` adds.  The trajectory has ``|node_to - node_from| + 1`` layers.  ``self.flow_trace_ms`` / ``self.flow_trace_bytes``:
        device milliseconds of the launches and the bytes copied to the host by the last call.  ``slide``: with the sliding mode
        (dots_flow_slide; the specification takes ``slide=True, areas=plan.area_tri``, the areas in the caller's numbering): the result
        gains ``"slides"`` and ``"steps"`` (P,) int32."""
        return self._flow("flow_trace", start_triangle, start_weights, neighbours, floor, max_crossings, trajectory, span=span, action=action,
                          slide=slide, mass=mass, attributes=attributes, exponents=exponents, layers=layers)

    def _flow(self, who, start_triangle, start_weights, neighbours, floor, max_crossings, trajectory, span=None, action=False, slide=False,
              mass=None, attributes=None, exponents=None, layers="end"):
        """What ``flow_map``, ``flow_push`` and ``flow_trace`` share; ``who`` names the method: it prefixes the messages, chooses the
        description and the entry point (``dots_<who>``; ``dots_flow_slide`` with ``slide``) and the ``<who>_ms`` / ``<who>_bytes`` set.
        Checks the arguments, allocates the result (``span`` None: the whole horizon), fills the embedded ``dots_flow_map_desc``
        wherever it sits in the description and, with a mass, the deposit fields, and brackets the call with the byte counter."""
        from . import flow

        if self.slab:
            raise ValueError(f"{who}: not available on time slabs")
        node_from, node_to = (0, self.T) if span is None else flow.check_span(span, self.T, who)
        if layers not in ("end", "all"):
            raise ValueError(f"{who}: layers must be 'end' or 'all'")
        tri = np.ascontiguousarray(start_triangle, dtype=np.int32)
        w = np.ascontiguousarray(start_weights, dtype=np.float64)
        nbr = np.ascontiguousarray(neighbours, dtype=np.int32)
        if tri.ndim != 1 or w.shape != (tri.shape[0], 3):
            raise ValueError(f"{who}: start_triangle (P,) and start_weights (P, 3) expected, got {tri.shape} and {w.shape}")
        if nbr.shape != (self.F, 3):
            raise ValueError(f"{who}: neighbours must have shape ({self.F}, 3), got {nbr.shape}")
        P, n = tri.shape[0], abs(node_to - node_from)
        out = {"triangle": np.empty(P, dtype=np.int32), "weights": np.empty((P, 3)), "status": np.empty(P, dtype=np.int32),
               "rested": np.empty(P, dtype=np.int32), "crossings": np.empty(P, dtype=np.int32)}
        if trajectory:
            out["triangles_at"] = np.empty((n + 1, P), dtype=np.int32)
            out["weights_at"] = np.empty((n + 1, P, 3))
        if action:
            out["action"] = np.empty(P)
        if slide:
            out["slides"], out["steps"] = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
        ms, dropped = C.c_double(), C.c_int64()
        # the description of the entry point: `whole` is passed, `d` holds the deposit fields, `m` is the embedded map description
        if who == "flow_map":
            whole = d = m = _lib.FlowMapDesc()
        elif who == "flow_push":
            whole = d = _lib.FlowPushDesc()
            m = d.map
        else:
            whole = _lib.FlowSlideDesc() if slide else _lib.FlowTraceDesc()
            d = whole.trace if slide else whole
            m = d.map
            d.node_from, d.node_to, d.action = node_from, node_to, _ptr(out.get("action"), C.c_double)
            if slide:
                whole.slides, whole.steps = _ptr(out["slides"], C.c_int32), _ptr(out["steps"], C.c_int32)
        m.n_particles, m.max_crossings, m.floor = P, int(max_crossings), float(floor)
        m.start_triangle, m.start_weights, m.neighbours = _ptr(tri, C.c_int32), _ptr(w, C.c_double), _ptr(nbr, C.c_int32)
        m.triangle, m.weights = _ptr(out["triangle"], C.c_int32), _ptr(out["weights"], C.c_double)
        m.status, m.rested, m.crossings = _ptr(out["status"], C.c_int32), _ptr(out["rested"], C.c_int32), _ptr(out["crossings"], C.c_int32)
        m.triangles_at, m.weights_at = _ptr(out.get("triangles_at"), C.c_int32), _ptr(out.get("weights_at"), C.c_double)
        m.ms = C.pointer(ms)
        push = who == "flow_push" or mass is not None
        if push:
            mass = np.ascontiguousarray(mass, dtype=np.float64)
            a = None if attributes is None else np.ascontiguousarray(attributes, dtype=np.float64)
            A = 0 if a is None else a.shape[0]
            if mass.shape != (P,) or (a is not None and (a.ndim != 2 or a.shape[1] != P)):
                raise ValueError(f"{who}: mass ({P},) and attributes (A, {P}) expected")
            k = np.ascontiguousarray(flow.push_scales(mass, a, w) if exponents is None else exponents, dtype=np.int32)
            if k.shape != (1 + A,):
                raise ValueError(f"{who}: {1 + A} exponents expected, got {k.shape}")
            L = n + 1 if layers == "all" else 1
            out["mass_at"] = np.empty((L, self.V))
            out["attr_at"] = np.empty((A, L, self.V)) if A else None
            d.mass, d.n_attributes, d.all_layers = _ptr(mass, C.c_double), A, int(layers == "all")
            d.attributes, d.scale_exponent = _ptr(a, C.c_double), _ptr(k, C.c_int32)
            d.mass_at, d.attr_at = _ptr(out["mass_at"], C.c_double), _ptr(out["attr_at"], C.c_double)
            d.dropped = C.pointer(dropped)
        elif attributes is not None or exponents is not None:
            raise ValueError(f"{who}: attributes and exponents need a mass")
        entry = "dots_flow_slide" if slide else "dots_" + who
        before = self.debug_counter(9)
        _lib.check(getattr(self.lib, entry)(self._h, C.byref(whole)), entry)
        setattr(self, who + "_ms", ms.value)
        setattr(self, who + "_bytes", self.debug_counter(9) - before)
        if push:
            out["dropped"], out["exponents"] = int(dropped.value), k
        return out

    def _carry_from(self, who, src, entry, describe, factors, same_grid):
        """What the three carriers share: the guards (``same_grid``: one ``n_time``), ``describe()`` -- the method's own validation, giving
        its descriptor and the arrays it points to --, the factors, the call of ``entry`` and its check.  Returns the launches' milliseconds."""
        if self.slab or src.slab:
            raise ValueError(f"{who}: not available on time slabs")
        if same_grid and self.T != src.T:
            raise ValueError(f"{who}: n_time = {self.T}, the source's {src.T}: both levels have one time grid")
        d, _arrays = describe()      # (_arrays: alive until the call has returned)
        for i, f in enumerate(factors):
            d.factor[i] = float(f)
        ms = C.c_double()
        d.ms = C.pointer(ms)
        _lib.check(getattr(self.lib, entry)(self._h, src._h, C.byref(d)), entry)
        return ms.value

    def _state_pitch(self):
        return max(8, 1 << int(np.ceil(np.log2(self.T + 1))))

    def _time_tables(self, src, d):
        """The time tables of ``d`` from ``src``'s grid to this one's; returns the arrays ``d`` points to."""
        from . import cascade

        nj, nw = cascade.time_weights(src.T, self.T, node=True)
        ij, iw = cascade.time_weights(src.T, self.T, node=False)
        d.node_j, d.node_w, d.interval_j, d.interval_w = _ptr(nj, C.c_int32), _ptr(nw, C.c_double), _ptr(ij, C.c_int32), _ptr(iw, C.c_double)
        return nj, nw, ij, iw

    def _space_tables(self, who, src, parents, transfer, size_first=True):
        """``(vsrc, vw, fsrc, csrc)`` in the two device numberings from ``parents`` (``vw`` and ``csrc`` None) or from ``transfer``.
        ``who``: what the message says where the map is not one to this context's mesh; ``size_first``: before the tables are made."""
        from . import cascade

        perms = (self.plan.perm_vert, self.plan.perm_tri, src.plan.perm_vert, src.plan.perm_tri)
        if parents is not None:
            v, t = cascade.check_parents(parents, n_vertices=src.V, n_triangles=src.F)
        else:
            v, _, t, _ = cascade.check_transfer(transfer, n_vertices=src.V, n_triangles=src.F)
        wrong = None if (v.shape[0], t.shape[0]) == (self.V, self.F) else f"{who} with V, F = {v.shape[0]}, {t.shape[0]}, this one has {self.V}, {self.F}"
        if wrong and size_first:
            raise ValueError(wrong)
        tables = cascade.transfer_row_maps(transfer, *perms) if parents is None else cascade.space_row_maps(parents, src.V, src.F, *perms)
        if wrong:
            raise ValueError(wrong)
        return tables if parents is None else (tables[0], None, tables[1], None)

    def _state_rows(self, per_vertex=1, per_triangle=1):
        """Rows of the twelve state arrays: 8 vertex arrays of V rows, 2 x 3 F triangle rows, 2 x 18 F corner rows."""
        return 8 * per_vertex * self.V + (2 * 3 + 2 * 18) * per_triangle * self.F

    def prolong_from(self, src: "DeviceProblem", factors=(1.0, 1.0, 1.0, 1.0)):
        """Fill this context's twelve state arrays with those of ``src`` (the same mesh on the same device, another ``n_time``,
        possibly another device numbering) interpolated linearly in time on the device (dots_prolong_time; cascade.prolong_time is
        the specification).  ``factors``: what the source values of (phi, A, B, lambda_c), the z arrays, (mu, E) and the beta arrays
        are multiplied with first -- the four factors of ``AlmSolver.recovered``.  Returns the milliseconds of the launches."""
        from . import cascade

        def describe():
            if (self.V, self.F) != (src.V, src.F):
                raise ValueError(f"prolong_from: another mesh (V, F = {self.V}, {self.F}, the source's {src.V}, {src.F})")
            d = _lib.ProlongDesc()
            tables = self._time_tables(src, d)
            vmap = cascade.row_map(self.plan.perm_vert, src.plan.perm_vert, self.V)
            fmap = cascade.row_map(self.plan.perm_tri, src.plan.perm_tri, self.F)
            d.vmap, d.fmap = _ptr(vmap, C.c_int32), _ptr(fmap, C.c_int32)
            return d, (tables, vmap, fmap)

        return self._carry_from("prolong_from", src, "dots_prolong_time", describe, factors, same_grid=False)

    def prolong_space_from(self, src: "DeviceProblem", parents, factors=(1.0, 1.0, 1.0, 1.0)):
        """Fill this context's twelve state arrays from those of ``src``, a context on the parent mesh of this one (``parents``:
        ``meshes.subdivide``) with the same ``n_time`` on the same device (dots_prolong_space; cascade.prolong_space is the
        specification).  ``factors``: as for ``prolong_from``.  Returns the milliseconds of the launches; ``self.prolong_bytes``: the
        bytes the transfer reads and writes when every source row is read once."""
        def describe():
            vmap, _, fmap, _ = self._space_tables("prolong_space_from: parents of a mesh", src, parents, None)
            d = _lib.ProlongSpaceDesc()
            d.vmap, d.fmap, d.n_vertices, d.n_triangles = _ptr(vmap, C.c_int32), _ptr(fmap, C.c_int32), self.V, self.F
            return d, (vmap, fmap)

        ms = self._carry_from("prolong_space_from", src, "dots_prolong_space", describe, factors, same_grid=True)
        self.prolong_bytes = 8 * self._state_pitch() * (self._state_rows() + src._state_rows())
        return ms

    def transfer_space_from(self, src: "DeviceProblem", transfer, factors=(1.0, 1.0, 1.0, 1.0)):
        """Fill this context's twelve state arrays from those of ``src``, a context on another triangulation of the same surface
        (``transfer``: ``cascade.mesh_transfer`` from its mesh to this one) with the same ``n_time`` on the same device
        (dots_transfer_space; cascade.transfer_space is the specification).  ``factors``: as for ``prolong_from``.  Returns the
        milliseconds of the launches; ``self.prolong_bytes``: one pass over this context's state (8 vertex arrays of V rows, 2 x 3 F
        triangle rows, 2 x 18 F corner rows, ``pitch`` doubles each), plus three source rows per vertex row, plus one source row per
        triangle / corner row: ``8 * pitch * (8 * V * (1 + 3) + 42 * F * (1 + 1))`` -- every source read counted, also those that
        come from the cache."""
        def describe():
            tables = self._space_tables("transfer_space_from: a transfer to a mesh", src, None, transfer)
            d = _lib.TransferSpaceDesc()
            d.vsrc, d.vw, d.fsrc, d.csrc = (_ptr(t, c) for t, c in zip(tables, (C.c_int32, C.c_double, C.c_int32, C.c_int32)))
            d.n_vertices, d.n_triangles = self.V, self.F
            return d, tables

        ms = self._carry_from("transfer_space_from", src, "dots_transfer_space", describe, factors, same_grid=True)
        self.prolong_bytes = 8 * self._state_pitch() * self._state_rows(1 + 3, 1 + 1)
        return ms

    def carry_spacetime_from(self, src: "DeviceProblem", factors=(1.0, 1.0, 1.0, 1.0), parents=None, transfer=None):
        """Fill this context's twelve state arrays from those of ``src``, a context on another mesh -- the parent mesh of this one
        (``parents``: ``meshes.subdivide``) or another triangulation of the same surface (``transfer``: ``cascade.mesh_transfer``),
        exactly one of the two -- AND at another ``n_time``, on the same device, in one pass (dots_carry_spacetime;
        cascade.carry_spacetime is the specification: space first, then time).  ``factors``: as for ``prolong_from``.  Returns the
        milliseconds of the launches; ``self.prolong_bytes``: one pass over this context's state at its own pitch, plus the source
        rows at the source's pitch -- nested, the source's state once (siblings share their source rows); located, three source rows
        per vertex row and one per triangle / corner row, every read counted."""
        from . import cascade

        def describe():
            cascade._one_map("carry_spacetime_from", parents, transfer)
            if self.T == src.T:
                raise ValueError(f"carry_spacetime_from: both contexts have n_time = {self.T}: on one time grid prolong_space_from / "
                                 "transfer_space_from are the definition")
            space = self._space_tables("carry_spacetime_from: a map to a mesh", src, parents, transfer, size_first=False)
            d = _lib.CarrySpacetimeDesc()
            time = self._time_tables(src, d)
            d.vsrc, d.vw, d.fsrc, d.csrc = (_ptr(t, c) for t, c in zip(space, (C.c_int32, C.c_double, C.c_int32, C.c_int32)))
            d.n_vertices, d.n_triangles = self.V, self.F
            return d, (time, space)

        ms = self._carry_from("carry_spacetime_from", src, "dots_carry_spacetime", describe, factors, same_grid=False)
        src_rows = src._state_rows() if parents is not None else self._state_rows(3, 1)
        self.prolong_bytes = 8 * (self._state_pitch() * self._state_rows() + src._state_pitch() * src_rows)
        return ms

    # ---- solve session: the next problem on this context
    def restart(self, mu0, mu1, mode="cold", factors=None, device_pointers=False, device_order=False):
        """Take the end masses of another problem on the same surface and start over on the live context (dots_restart): the factor,
        the hierarchy and every allocation are kept, the parameters go back to a new context's (``self.params`` is read again).
        ``mode="cold"``: the state is zeroed; ``"warm"``: every state array is multiplied in place by its entry of ``factors``, the
        four of ``AlmSolver.recovery_factors()`` -- the bits that downloading, ``recovered`` and ``init_solution=`` leave.  ``mu0`` /
        ``mu1`` (V,) in the caller's numbering: arrays, or with ``device_pointers`` torch tensors on the context's device (permuted
        there; nothing crosses to the host except that ``self.plan``'s copies are refreshed for ``_initial_constant_scaling``).
        ``device_order`` (with ``device_pointers``): the tensors are in the CONTEXT's vertex numbering already, where
        ``barycenter_update`` writes ``nu_device_order``: they are read as they are, nothing is permuted and nothing is copied to the
        host -- ``self.plan`` then holds no end masses (None), and a run that reads them there (``is_constant_scaling``) cannot start.
        Returns the device milliseconds of the call."""
        if self.slab:
            raise ValueError("restart: not available on time slabs")
        if device_order and not device_pointers:
            raise ValueError("restart: device_order is for tensors on the device (device_pointers)")
        if mode not in ("cold", "warm"):
            raise ValueError("restart: mode must be 'cold' or 'warm'")
        if mode == "warm" and (factors is None or len(factors) != 4):
            raise ValueError("restart: a warm restart needs the four recovery factors")
        perm = self.plan.perm_vert
        d = _lib.RestartDesc()
        if device_pointers:
            import torch

            where = torch.device("cuda", self.device)
            dev = []
            for name, a in (("mu0", mu0), ("mu1", mu1)):
                if not isinstance(a, torch.Tensor) or a.device != where or a.dtype != torch.float64 or tuple(a.shape) != (self.V,):
                    raise ValueError(f"restart: {name} must be a float64 tensor of shape ({self.V},) on {where}")
                a = a.detach()
                dev.append((a if perm is None or device_order else a[torch.as_tensor(perm, device=where, dtype=torch.int64)]).contiguous())
            torch.cuda.current_stream(where).synchronize()      # (the call reads them on the context's stream)
            d.mu0, d.mu1 = dev[0].data_ptr(), dev[1].data_ptr()
            host = [None, None] if device_order else [t.cpu().numpy() for t in dev]
        else:
            host = []
            for name, a in (("mu0", mu0), ("mu1", mu1)):
                a = np.asarray(a, dtype=np.float64)
                if a.shape != (self.V,):
                    raise ValueError(f"restart: {name} must have shape ({self.V},), got {a.shape}")
                host.append(np.ascontiguousarray(a if perm is None else a[perm]))
            d.mu0, d.mu1 = host[0].ctypes.data, host[1].ctypes.data
        d.device_pointers, d.mode = int(bool(device_pointers)), _lib.RESTART_WARM if mode == "warm" else _lib.RESTART_COLD
        for i in range(4):
            d.factors[i] = float(factors[i]) if mode == "warm" else 1.0
        ms = C.c_double()
        d.ms = C.pointer(ms)
        _lib.check(self.lib.dots_restart(self._h, C.byref(d)), "dots_restart")
        import dataclasses

        self.plan = dataclasses.replace(self.plan, mu0=host[0], mu1=host[1])      # (shared plans of other solvers keep theirs)
        _lib.check(self.lib.dots_get_params(self._h, C.byref(self.params)), "dots_get_params")
        self.restart_ms = ms.value
        return ms.value

    def barycenter_update(self, potentials, weights, eta, mass, nu, nu_device_order=None):
        """One mirror-descent step of a barycentre on this context's surface and device (``barycenter_update`` below with the
        context's vertex numbering): ``nu_device_order`` receives ``nu`` in the numbering ``restart(device_pointers=True,
        device_order=True)`` reads.  The context itself is not involved -- the library call takes none --: its iterate, parameters and
        stream are untouched.  ``self.barycenter_ms``: device milliseconds of the launches."""
        if self.slab:
            raise ValueError("barycenter_update: not available on time slabs")
        import torch

        if getattr(self, "_vertex_row", None) is None:      # caller vertex -> row of the context's numbering: the inverse of perm_vert
            perm = self.plan.perm_vert
            row = np.arange(self.V, dtype=np.int32)
            if perm is not None:
                row[np.asarray(perm, dtype=np.int64)] = np.arange(self.V, dtype=np.int32)
            self._vertex_row = torch.as_tensor(row, device=torch.device("cuda", self.device))
        scalars, self.barycenter_ms = barycenter_update(potentials, weights, eta, mass, nu, nu_device_order, self._vertex_row)
        return scalars

    # ---- linearised transport: the calls take no context; the context lends its surface and device
    def tangent_mesh(self):
        """The four mesh tensors of the ``tangent_*`` calls on the context's device, in the CALLER's numbering -- ``triangles`` (F, 3)
        int32, ``hat`` (F, 3, 3), ``area`` (F,), ``mass`` (V,) --, taken from the plan's host arrays (the ones the context was built
        from, permuted back) and cached until the plan changes (``move_vertices``)."""
        if self.slab:
            raise ValueError("tangent: not available on time slabs")
        cached = getattr(self, "_tangent_mesh", None)
        if cached is None or cached[0] is not self.plan:
            import torch

            self._tangent_mesh = cached = (self.plan, {k: torch.as_tensor(a, device=torch.device("cuda", self.device))
                                                       for k, a in caller_tables(self.plan).items()})
        return cached[1]

    def tangent_velocities(self, potentials):
        """``grad phi`` per triangle of every potential, (n, F, 3) on the device (``tangent_velocities`` below on this context's
        surface): ``potentials`` as ``sensitivity(to_device=True)`` left them.  ``self.tangent_ms["velocities"]``: device milliseconds."""
        out, ms = tangent_velocities(self.tangent_mesh(), potentials)
        self.tangent_ms = {**getattr(self, "tangent_ms", {}), "velocities": ms}
        return out

    def tangent_weights(self, sigma):
        """The mass of ``sigma`` (V,), a tensor on the device in the caller's numbering, on every triangle: (F,) on the device."""
        out, ms = tangent_weights(self.tangent_mesh(), sigma)
        self.tangent_ms = {**getattr(self, "tangent_ms", {}), "weights": ms}
        return out

    def tangent_gram(self, A, B, w):
        """The Gram matrix (na, nb) of the fields ``A`` and ``B`` (None: ``A``) with the triangle weights ``w``, all on the device;
        a host array: only it crosses."""
        out, ms = tangent_gram(A, B, w)
        self.tangent_ms = {**getattr(self, "tangent_ms", {}), "gram": ms}
        return out

    def move_vertices(self, vertices, device_pointers=False):
        """Move the vertices of the live context to ``vertices`` (V, 3), caller's numbering (dots_move_vertices): every geometry table
        is assembled again on the device and a factor the context owns is computed again into its allocations; the tree, the plan of
        the bands and the state stay.  The context then needs ``restart`` before it steps.  An array, or with ``device_pointers`` a
        float64 torch tensor on the context's device (permuted there; the positions come down once, 24 V bytes, for the plan).
        ``self.plan`` becomes ``geometry.plan_with_vertices(self.plan, vertices)`` and ``self.params`` is read again.  Returns the
        device milliseconds of the assembly launches, of the factor refresh and of the whole call."""
        d, ms, plan, keep = self._move_desc(vertices, device_pointers)
        _lib.check(self.lib.dots_move_vertices(self._h, C.byref(d)), "dots_move_vertices")
        return self._moved(plan, ms)

    def _move_desc(self, vertices, device_pointers):
        """The descriptor of a move to ``vertices`` (permuted into this context's numbering), its ``ms`` array, the moved plan and what
        keeps the descriptor's memory alive: ``move_vertices`` and ``move_vertices_many``."""
        from .geometry import plan_with_vertices

        if self.slab:
            raise ValueError("move_vertices: not available on time slabs")
        perm = self.plan.perm_vert
        d = _lib.MoveDesc()
        if device_pointers:
            import torch

            where = torch.device("cuda", self.device)
            a = vertices
            if not isinstance(a, torch.Tensor) or a.device != where or a.dtype != torch.float64 or tuple(a.shape) != (self.V, 3):
                raise ValueError(f"move_vertices: vertices must be a float64 tensor of shape ({self.V}, 3) on {where}")
            a = a.detach()
            keep = (a if perm is None else a[torch.as_tensor(perm, device=where, dtype=torch.int64)]).contiguous()
            torch.cuda.current_stream(where).synchronize()      # (the call reads it on the context's stream)
            d.vertices = keep.data_ptr()
            host = a.cpu().numpy()
        else:
            host = np.asarray(vertices, dtype=np.float64)
            if host.shape != (self.V, 3):
                raise ValueError(f"move_vertices: vertices must have shape ({self.V}, 3), got {host.shape}")
            keep = np.ascontiguousarray(host if perm is None else host[perm])
            d.vertices = keep.ctypes.data
        plan = plan_with_vertices(self.plan, host)      # (raises for what the library would refuse, before the context is touched)
        d.device_pointers = int(bool(device_pointers))
        ms = (C.c_double * 3)()
        d.ms = C.cast(ms, C.POINTER(C.c_double))
        return d, ms, plan, keep

    def _moved(self, plan, ms):
        self.plan = plan
        _lib.check(self.lib.dots_get_params(self._h, C.byref(self.params)), "dots_get_params")
        self.move_ms = tuple(float(x) for x in ms)
        return self.move_ms

    def geometry_tables(self):
        """The geometry tables the context holds (dots_geometry_copy), device numbering: a dict of arrays named as ``DevicePlan``'s,
        plus ``kdiag`` (V,), ``corner_scale`` (3F,) and ``corner_grad_area`` (3F, 3) in corner-list order."""
        V, F, nnz = self.V, self.F, int(self.plan.lap_val.size)
        out = {"area_tri": np.empty(F), "hat_grad": np.empty((F, 3, 3)), "mass_vert": np.empty(V), "lap_val": np.empty(nnz), "kdiag": np.empty(V),
               "corner_scale": np.empty(3 * F), "corner_grad_area": np.empty((3 * F, 3))}
        t = _lib.GeometryTables()
        for name, a in out.items():
            setattr(t, name, _ptr(a, C.c_double))
        _lib.check(self.lib.dots_geometry_copy(self._h, C.byref(t)), "dots_geometry_copy")
        return out

    # ---- the hot loop
    def step(self, n_iters=1, wait=True):
        """``wait=False``: only enqueue (direct solver); returns None, nothing is timed."""
        if not wait:
            _lib.check(self.lib.dots_step(self._h, int(n_iters), None), "dots_step")
            return None
        st = _lib.StepStats()
        _lib.check(self.lib.dots_step(self._h, int(n_iters), C.byref(st)), "dots_step")
        return st

    def step_flags(self, skip_z_mid=False, palm=False, rhs_ahead=False, timed=False, carry=False, kkt_sums=False):
        """``rhs_ahead`` (DOTS_STEP_RHS_AHEAD): the first KKT read-back after the next step also enqueues the right-hand side of
        the iteration after it; only meaningful with the direct solver on one GPU.  ``timed`` (DOTS_STEP_TIMED): enqueue-only
        steps record phase events that ``step_times`` collects later.  ``carry`` (DOTS_STEP_CARRY): the next iteration starts
        from the state this one leaves, so steps 2+3 also store the per-corner sums its right-hand side and projection gather.
        ``kkt_sums`` (DOTS_STEP_KKT_SUMS): residuals are read after the step; steps 2+3 also form the sums of conditions 0, 1, 3, 6."""
        flags = ((_lib.STEP_SKIP_Z_MID if skip_z_mid else 0) | (_lib.STEP_PALM if palm else 0) | (_lib.STEP_RHS_AHEAD if rhs_ahead else 0)
                 | (_lib.STEP_TIMED if timed else 0) | (_lib.STEP_CARRY if carry else 0) | (_lib.STEP_KKT_SUMS if kkt_sums else 0))
        _lib.check(self.lib.dots_step_flags(self._h, flags), "dots_step_flags")

    def penalty_ahead(self, tol, is_org_kkt, r_lower, r_upper, table):
        """dots_penalty_ahead: the next evaluation of conditions 0-3 takes the reference's penalty decision inside the library and starts
        the next iteration's first launch with it (``table``: (threshold, factor) pairs of admm_tools.py:79-90); a hint."""
        pol = getattr(self, "_penalty_policy", None)
        if pol is None:
            pol = self._penalty_policy = _lib.PenaltyPolicy()
            pol.n_steps = len(table)
            for i, (bound, val) in enumerate(table):
                pol.threshold[i], pol.factor[i] = bound, val
        pol.tol, pol.r_lower, pol.r_upper, pol.is_org_kkt = float(tol), float(r_lower), float(r_upper), 1 if is_org_kkt else 0
        _lib.check(self.lib.dots_penalty_ahead(self._h, C.byref(pol)), "dots_penalty_ahead")

    def step_times(self, wait=False, capacity=64):
        """Phase times of the timed enqueue-only steps that have finished (``wait``: of all of them), oldest first."""
        buf = getattr(self, "_times_buf", None)
        if buf is None or len(buf) < capacity:
            buf = self._times_buf = (_lib.StepStats * capacity)()
        n = C.c_int(0)
        _lib.check(self.lib.dots_step_times(self._h, buf, capacity, 1 if wait else 0, C.byref(n)), "dots_step_times")
        out = []
        for i in range(n.value):       # copies: the buffer is reused by the next call
            st = _lib.StepStats()
            C.pointer(st)[0] = buf[i]
            out.append(st)
        return out

    # ---- time slab (multi-GPU): stages of one iteration around the caller's exchanges (dots_slab_stage)
    def slab_elems(self, which):
        return int(self.lib.dots_slab_elems(self._h, _lib.SLAB_SIZES[which]))

    def slab_set_buffers(self, **pointers):
        b = _lib.SlabBuffers()
        for name in _lib.SlabBuffers.NAMES:
            setattr(b, name, int(pointers[name]))
        _lib.check(self.lib.dots_slab_set_buffers(self._h, C.byref(b)), "dots_slab_set_buffers")

    def slab_stage(self, stage, wait=False):
        """``wait=False``: only enqueue on the context's stream (order the exchange with ``stream_wait``)."""
        st = _lib.StepStats() if wait else None
        _lib.check(self.lib.dots_slab_stage(self._h, int(stage), C.byref(st) if wait else None), f"dots_slab_stage {stage}")
        return st

    def stream_wait(self, other_stream, ctx_waits):
        """Order the context's stream against another HIP stream (an integer handle, 0 = default stream)."""
        _lib.check(self.lib.dots_stream_wait(self._h, C.c_void_p(int(other_stream)), 1 if ctx_waits else 0), "dots_stream_wait")

    def run_phase(self, phase):
        st = _lib.StepStats()
        _lib.check(self.lib.dots_run_phase(self._h, _lib.PHASES[phase], C.byref(st)), f"phase {phase}")
        return st

    def kkt(self, conditions):
        """Evaluate the listed KKT conditions; returns {i: [value, value_at_unit_scale or None]}."""
        mask = 0
        for i in conditions:
            mask |= 1 << int(i)
        out = getattr(self, "_kkt_out", None)      # (the host's part of a read-back sits on the critical path: no allocations here)
        if out is None:
            out = self._kkt_out = np.empty(14)
            self._kkt_out_p = _ptr(out, C.c_double)
        out.fill(np.nan)
        _lib.check(self.lib.dots_kkt(self._h, mask, self._kkt_out_p), "dots_kkt")
        vals = out.tolist()
        return {int(i): [vals[2 * i], None if i >= 4 else vals[2 * i + 1]] for i in conditions}

    @staticmethod
    def _mask(conditions):
        mask = 0
        for i in conditions:
            mask |= 1 << int(i)
        return mask

    def kkt_sums(self, conditions):
        """The weighted sums of this context's time slab that the listed conditions need (to be added over the slabs)."""
        sums = np.zeros(_lib.KKT_N_SUMS)
        _lib.check(self.lib.dots_kkt_sums(self._h, self._mask(conditions), _ptr(sums, C.c_double)), "dots_kkt_sums")
        return sums

    def kkt_sums_device(self, conditions, device_ptr):
        """``kkt_sums`` left in the caller's DEVICE buffer of ``KKT_N_SUMS`` doubles (an integer address, e.g. a torch
        tensor's ``data_ptr()``): only enqueued on the context's stream -- order the consumer with ``stream_wait``."""
        _lib.check(self.lib.dots_kkt_sums_device(self._h, self._mask(conditions), C.c_void_p(int(device_ptr))), "dots_kkt_sums_device")

    def debug_counter(self, which=0):
        return int(self.lib.dots_debug_counter(self._h, int(which)))

    def kkt_combine(self, conditions, sums):
        """The listed KKT residuals from the sums of the whole problem; same return value as ``kkt``."""
        out = np.full(14, np.nan)
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        _lib.check(self.lib.dots_kkt_combine(self._h, self._mask(conditions), _ptr(sums, C.c_double), _ptr(out, C.c_double)), "dots_kkt_combine")
        return {int(i): [float(out[2 * i]), None if i >= 4 else float(out[2 * i + 1])] for i in conditions}

    def objective(self):
        out = np.zeros(2)
        _lib.check(self.lib.dots_objective(self._h, _ptr(out, C.c_double)), "dots_objective")
        return float(out[0]), float(out[1])

    def objective_sums(self):
        sums = np.zeros(3)
        _lib.check(self.lib.dots_objective_sums(self._h, _ptr(sums, C.c_double)), "dots_objective_sums")
        return sums

    def objective_combine(self, sums):
        out, sums = np.zeros(2), np.ascontiguousarray(sums, dtype=np.float64)
        _lib.check(self.lib.dots_objective_combine(self._h, _ptr(sums, C.c_double), _ptr(out, C.c_double)), "dots_objective_combine")
        return float(out[0]), float(out[1])

    def adjust_penalty(self, factor):
        _lib.check(self.lib.dots_adjust_penalty(self._h, float(factor)), "dots_adjust_penalty")

    def scale_z(self, z_mul, beta_mul, scale_z_new):
        _lib.check(self.lib.dots_scale_z(self._h, float(z_mul), float(beta_mul), float(scale_z_new)), "dots_scale_z")

    def scale_arrays(self, names, factor):
        mask = 0
        for n in names:
            mask |= 1 << _lib.ARRAY_IDS[n]
        _lib.check(self.lib.dots_scale_arrays(self._h, mask, float(factor)), "dots_scale_arrays")

    def norm_square(self, name, part=0):
        out = C.c_double()
        _lib.check(self.lib.dots_norm_square(self._h, _lib.ARRAY_IDS[name], int(part), C.byref(out)), "dots_norm_square")
        return out.value

    def apply_operator(self, op, x, scale=1.0):
        shapes = {
            "grad_time": ("phi", "A"), "div_time": ("A", "phi"), "time_avg_adjoint": ("A", "phi"),
            "grad_space": ("phi", "B"), "div_space": ("B", "phi"), "decouple": ("B", "z_mid"),
            "decouple_adjoint": ("z_mid", "B"), "laplacian_apply": ("phi", "phi"),
        }
        sin, sout = shapes[op]
        a = np.ascontiguousarray(x, dtype=np.float64)
        if a.shape != self.shape(sin):
            raise ValueError(f"{op}: expected input shape {self.shape(sin)}, got {a.shape}")
        out = np.empty(self.shape(sout), dtype=np.float64)
        _lib.check(
            self.lib.dots_apply_operator(self._h, _lib.OPERATORS[op], float(scale), _ptr(a, C.c_double), a.size,
                                         _ptr(out, C.c_double), out.size),
            f"operator {op}",
        )
        return out

    # ---- multigrid preconditioner of the modal PCG
    def setup_multigrid(self, eps=0.0, omega=2.0 / 3.0, coarsest=256, mode_slice=None):
        """Build the smoothed-aggregation hierarchy on the host and upload it (see multigrid.py).

        ``mode_slice``: the time modes this context solves (default: all T+1).  Returns the
        hierarchy summary, or None when the mesh is too small for a second level (Jacobi stays)."""
        import scipy.sparse as sp

        from . import multigrid

        if self.lap_solver != "modal_pcg":
            raise ValueError("the multigrid preconditioner needs lap_solver='modal_pcg'")
        p = self.plan
        K = sp.csr_matrix((p.lap_val, p.lap_col, p.lap_rowptr), shape=(p.n_vertices, p.n_vertices))
        levels = multigrid.build_hierarchy(K, p.mass_vert, coarsest=coarsest)
        if len(levels) < 2:
            return None
        if mode_slice is None:
            mode_slice = self.mode_slice
        sigma = p.time_eigs if mode_slice is None else p.time_eigs[mode_slice]
        if sigma.size == 0:
            return None      # a rank without modes solves nothing
        last = levels[-1]
        inv = np.empty((last.n, last.n, sigma.size))
        # one block of modes per window of the PCG (one window up to 256 modes; a time slab's slice is one too): the library installs
        # the coarse inverse window by window from this array
        windows = pcg_window_plan(self.T) if (getattr(self, "pcg_windows", False) and mode_slice is None) else [(0, sigma.size)]
        for first, live in windows:
            for k in range(first, first + live):
                inv[:, :, k] = multigrid.coarse_inverse(last, float(sigma[k] + eps))
        keep = []   # host arrays must stay alive until dots_mg_setup returns

        def arr(a, dtype):
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            return a

        lv = (_lib.MgLevel * len(levels))()
        for l, L in enumerate(levels):
            h = lv[l]
            h.n = L.n
            if l > 0:
                h.nnz = int(L.K.nnz)
                h.rowptr = _ptr(arr(L.K.indptr, np.int32), C.c_int32)
                h.col = _ptr(arr(L.K.indices, np.int32), C.c_int32)
                h.val_k = _ptr(arr(L.K.data, np.float64), C.c_double)
                h.val_m = _ptr(arr(L.M.data, np.float64), C.c_double)
                h.diag_k = _ptr(arr(L.dK, np.float64), C.c_double)
                h.diag_m = _ptr(arr(L.dM, np.float64), C.c_double)
            if L.P is not None:
                h.n_coarse = L.P.shape[1]
                h.p_nnz = int(L.P.nnz)
                h.p_rowptr = _ptr(arr(L.P.indptr, np.int32), C.c_int32)
                h.p_col = _ptr(arr(L.P.indices, np.int32), C.c_int32)
                h.p_val = _ptr(arr(L.P.data, np.float64), C.c_double)
                h.r_rowptr = _ptr(arr(L.R.indptr, np.int32), C.c_int32)
                h.r_col = _ptr(arr(L.R.indices, np.int32), C.c_int32)
                h.r_val = _ptr(arr(L.R.data, np.float64), C.c_double)
                h.ap_nnz = int(L.KP.nnz)
                h.ap_rowptr = _ptr(arr(L.KP.indptr, np.int32), C.c_int32)
                h.ap_col = _ptr(arr(L.KP.indices, np.int32), C.c_int32)
                h.ap_val_k = _ptr(arr(L.KP.data, np.float64), C.c_double)
                h.ap_val_m = _ptr(arr(L.MP.data, np.float64), C.c_double)
                h.ap_val_p = _ptr(arr(L.PP.data, np.float64), C.c_double)
        desc = _lib.MgDesc()
        desc.n_levels = len(levels)
        desc.n_cols = int(sigma.size)
        desc.omega = float(omega)
        desc.levels = lv
        desc.coarse_inverse = _ptr(arr(inv, np.float64), C.c_double)
        _lib.check(self.lib.dots_mg_setup(self._h, C.byref(desc)), "dots_mg_setup")
        self.mg_levels = levels      # exactly what was uploaded (the plan's vertex numbering): the host reference of mg_apply runs on these
        self.mg_summary = multigrid.hierarchy_summary(levels)
        return self.mg_summary

    def mg_apply(self, r, frozen=None):
        """ONE V-cycle of the installed hierarchy on the residual ``r`` (``(T+1, V)``: modes x vertices, the caller's numbering), with
        the launches the PCG uses; ``frozen``: modes to skip (their ``z`` stays ``D^-1 r``).  Returns ``(z, rz)``, ``rz[a] = r[a] . z[a]``
        summed from the per-workgroup partial sums.  For tests and diagnosis: the solver never calls it.  ``mg_path()`` then tells
        which kernels ran."""
        a = np.ascontiguousarray(r, dtype=np.float64)
        if a.shape != (self.T + 1, self.V):
            raise ValueError(f"mg_apply: expected r of shape {(self.T + 1, self.V)}, got {a.shape}")
        fp = None
        if frozen is not None:
            f = np.ascontiguousarray(np.asarray(frozen) != 0, dtype=np.int32)
            if f.shape != (self.T + 1,):
                raise ValueError(f"mg_apply: expected {self.T + 1} frozen marks, got shape {f.shape}")
            fp = _ptr(f, C.c_int32)
        z, rz = np.empty_like(a), np.empty(self.T + 1)
        _lib.check(self.lib.dots_mg_apply(self._h, _ptr(a, C.c_double), _ptr(z, C.c_double), _ptr(rz, C.c_double), fp), "dots_mg_apply")
        return z, rz

    def mg_path(self):
        """Names of the launches the last V-cycle took and the number of levels inside its tail launch (``_lib.MG_PATH``)."""
        mask = self.debug_counter(_lib.MG_PATH_COUNTER)
        return {n for n, bit in _lib.MG_PATH.items() if mask & bit}, (mask >> _lib.MG_PATH_TAIL_LEVELS_SHIFT) & 15

    def cg_path(self):
        """``(names, vt, cap, G)`` of the last launches of the PCG kernels (``_lib.CG_PATH``): the path bits that are set, the vertices
        per tile, the CSR entries of a tile staged in LDS and the number of workgroups; ``(set(), 0, 0, 0)`` before the first."""
        mask = self.debug_counter(_lib.CG_PATH_COUNTER)
        return ({n for n, bit in _lib.CG_PATH.items() if mask & bit}, (mask >> _lib.CG_PATH_VT_SHIFT) & 0xfff,
                (mask >> _lib.CG_PATH_CAP_SHIFT) & 0xfff, mask >> _lib.CG_PATH_G_SHIFT)

    # ---- direct (multifrontal) solve of the modal problems
    def setup_frontal(self, eps=0.0, leaf=None, mode_slice=None, numeric="device", bands=None, top_inverse=None):
        """Factorise K + (sigma_a + eps) M for this context's modes on one nested-dissection tree
        (frontal.py) and install the factor: step 1 then runs two triangular sweeps instead of the PCG.
        ``numeric``: "device" (HIP kernels, the default) or "host" (numpy reference, small meshes only).
        ``bands``: tree heights one launch of a sweep handles, ``top_inverse``: the top band as explicit inverses, one launch
        for both sweeps (frontal.plan_bands; default: the plan's own choice)."""
        import scipy.sparse as sp

        from . import frontal

        if self.lap_solver != "modal_pcg":
            raise ValueError("the direct solve needs the modal solver")
        p = self.plan
        K = sp.csr_matrix((p.lap_val, p.lap_col, p.lap_rowptr), shape=(p.n_vertices, p.n_vertices))
        diss = p.dissection if leaf is None else None     # the plan's own tree (reorder="nd") unless a leaf size is forced
        if diss is None:
            diss = frontal.nested_dissection(K.indptr, K.indices, p.vertices, leaf=leaf or 16)
        if mode_slice is None:
            mode_slice = self.mode_slice
        sigma = p.time_eigs if mode_slice is None else p.time_eigs[mode_slice]
        if sigma.size == 0:
            return None
        pitch = int(self.lib.dots_front_pitch(self._h))
        p_pitch = max(8, 1 << int(np.ceil(np.log2(p.n_time + 1))))     # the whole problem's pitch (a time slab's own one is smaller)
        if numeric not in ("device", "host"):
            raise ValueError("numeric must be 'device' or 'host'")
        self.set_params(eps=float(eps))      # the device factorisation reads eps from the context
        ff = frontal.factorize(K, p.mass_vert, sigma + float(eps), diss, pitch=pitch, numeric=numeric == "host")
        if bands is None:
            if diss.bands is not None:
                bands, auto_top = diss.bands, diss.top_inverse
            else:
                bands, auto_top = frontal.plan_bands(diss, ff.node_n, ff.node_b, p_pitch)
            if top_inverse is None:
                top_inverse = auto_top
        bands = np.ascontiguousarray(bands, dtype=np.int32)
        d = _lib.FrontDesc()
        d.band_ptr, d.n_bands, d.top_inverse = _ptr(bands, C.c_int32), bands.size - 1, 1 if top_inverse else 0
        d.n_nodes, d.n_levels, d.n_modes, d.pitch = ff.node_n.size, ff.level_ptr.size - 1, ff.n_modes, ff.pitch
        d.n_front_rows, d.n_entries, d.update_rows = ff.front_idx.size, ff.stats["factor_entries_per_mode"], ff.update_rows
        flags = np.zeros(ff.n_modes, dtype=np.int32)
        flags[ff.grounded] = 1
        keep = [np.ascontiguousarray(a) for a in (ff.node_n, ff.node_b, ff.node_foff, ff.node_ioff, ff.node_uoff, ff.node_child,
                                                   ff.front_idx, ff.pull0, ff.pull1, ff.level_ptr, ff.level_nodes)]
        keep.append(None if ff.values is None else np.ascontiguousarray(ff.values))
        d.grounded = _ptr(flags, C.c_int32)
        d.node_n, d.node_b = _ptr(keep[0], C.c_int32), _ptr(keep[1], C.c_int32)
        d.node_foff, d.node_ioff, d.node_uoff = _ptr(keep[2], C.c_int64), _ptr(keep[3], C.c_int64), _ptr(keep[4], C.c_int64)
        d.node_child, d.front_idx = _ptr(keep[5], C.c_int32), _ptr(keep[6], C.c_int32)
        d.pull0, d.pull1 = _ptr(keep[7], C.c_int32), _ptr(keep[8], C.c_int32)
        d.level_ptr, d.level_nodes, d.values = _ptr(keep[9], C.c_int32), _ptr(keep[10], C.c_int32), _ptr(keep[11], C.c_double)
        _lib.check(self.lib.dots_front_setup(self._h, C.byref(d)), "dots_front_setup")
        self.front_summary = dict(ff.stats)
        self.front_summary["launches_per_solve"] = self.front_launches()
        info = (C.c_double * 4)()
        _lib.check(self.lib.dots_front_info(self._h, info), "dots_front_info")
        self.front_summary.update(bands=[int(x) for x in bands], top_inverse=bool(top_inverse), bytes_per_solve_one_block_per_node=float(info[0]),
                                  bytes_per_solve_as_installed=float(info[1]), leaf_inverse=self.debug_counter(4) > 0)
        return self.front_summary

    def share_frontal(self, owner: "DeviceProblem"):
        """Install the factor of ``owner`` (a context with ``setup_frontal`` done) in this context (dots_front_share): the factor is
        shared, reference-counted, this context allocates only the vectors one solve writes.  Same mesh in the same numbering (build
        the context on ``owner.plan`` or on ``geometry.plan_with_densities(owner.plan, ...)``) and the same eps in ``params``."""
        _lib.check(self.lib.dots_front_share(self._h, owner._h), "dots_front_share")
        self.front_summary = getattr(owner, "front_summary", None)
        return self.front_summary

    def front_launches(self):
        return int(self.lib.dots_front_launches(self._h))

    def enable_frontal(self, on=True):
        _lib.check(self.lib.dots_front_enable(self._h, 1 if on else 0), "dots_front_enable")

    def enable_pcg_windows(self, on=True):
        """dots_pcg_windows: above 256 time nodes and without an enabled factor, step 1 solves the time modes in windows of 256
        (``pcg_window_plan``) with the modal PCG instead of refusing.  Changing the setting above 256 nodes drops an installed
        multigrid hierarchy (``setup_multigrid`` again)."""
        _lib.check(self.lib.dots_pcg_windows(self._h, 1 if on else 0), "dots_pcg_windows")
        self.pcg_windows = bool(on)

    def pcg_windows_ran(self):
        """``(windows, transforms)``: the windows the last PCG solve ran (0: none yet, or it ran unwindowed) and whether the windowed
        time transforms ran (dots_debug_counter 14)."""
        mask = self.debug_counter(_lib.PCG_WINDOWS_COUNTER)
        return mask & 0xff, bool(mask & _lib.PCG_WINDOWS_TRANSFORMS)

    def enable_multigrid(self, on=True):
        _lib.check(self.lib.dots_mg_enable(self._h, 1 if on else 0), "dots_mg_enable")

    def bench_kernel(self, which=0, reps=50):
        ms, nbytes = C.c_double(), C.c_double()
        _lib.check(self.lib.dots_bench_kernel(self._h, int(which), int(reps), C.byref(ms), C.byref(nbytes)), "dots_bench_kernel")
        return ms.value, nbytes.value

    def sync(self):
        _lib.check(self.lib.dots_sync(self._h), "dots_sync")

    def device_bytes(self):
        return int(self.lib.dots_device_bytes(self._h))


def laplacian_solve_many(problems, arrays):
    """Step 1's operator inverse of ``arrays[k]`` ([T+1, V], reference layout) on ``problems[k]``, for problems that share one factor
    (``DeviceProblem.share_frontal``): ONE batched pair of sweeps for all of them (dots_laplacian_solve_many).  Returns the solutions,
    each bit for bit what the call on that problem alone returns."""
    problems = list(problems)
    if len(problems) != len(arrays) or not problems:
        raise ValueError("laplacian_solve_many: one array per problem, at least one problem")
    lib = problems[0].lib
    ins = []
    for p, a in zip(problems, arrays):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != p.shape("phi"):
            raise ValueError(f"laplacian_solve_many: expected shape {p.shape('phi')}, got {a.shape}")
        ins.append(a)
    outs = [np.empty(p.shape("phi"), dtype=np.float64) for p in problems]
    n = len(problems)
    hs = (C.c_void_p * n)(*[p._h.value for p in problems])
    pin = (C.POINTER(C.c_double) * n)(*[_ptr(a, C.c_double) for a in ins])
    pout = (C.POINTER(C.c_double) * n)(*[_ptr(a, C.c_double) for a in outs])
    _lib.check(lib.dots_laplacian_solve_many(hs, n, pin, pout), "dots_laplacian_solve_many")
    return outs


def _handles(problems):
    problems = list(problems)
    if not problems:
        raise ValueError("at least one problem")
    return problems, (C.c_void_p * len(problems))(*[p._h.value for p in problems])


def step_many(problems, stats=False):
    """One ALM iteration of every problem (they share one factor), each under its own step flags, with ONE batched pair of sweeps
    (dots_step_many).  ``stats``: the host waits and the batch's phase times come back as a ``StepStats``; otherwise the iteration is only
    enqueued and None is returned."""
    problems, hs = _handles(problems)
    st = _lib.StepStats() if stats else None
    _lib.check(problems[0].lib.dots_step_many(hs, len(problems), C.byref(st) if stats else None), "dots_step_many")
    return st


def move_vertices_many(problems, vertices, device_pointers=False):
    """Move the vertices of every problem to ``vertices`` (V, 3), caller's numbering (dots_move_vertices_many).  ``problems`` are ALL
    the holders of one factor (``DeviceProblem.share_frontal``), built on one plan up to the densities: every member's geometry tables
    are assembled again, the factor is computed again ONCE into the allocations it has, and each member then needs ``restart``
    before it steps.  ``vertices`` as for ``DeviceProblem.move_vertices``.  Every member's ``plan`` becomes the moved plan with its
    own densities and its ``params`` are read again.  Returns the device milliseconds of the assembly launches (summed over the
    members), of the one factor refresh and of the whole call, which is also every member's ``move_ms``."""
    import dataclasses

    problems, hs = _handles(problems)
    d, ms, plan, keep = problems[0]._move_desc(vertices, device_pointers)
    _lib.check(problems[0].lib.dots_move_vertices_many(hs, len(problems), C.byref(d)), "dots_move_vertices_many")
    for p in problems:
        out = p._moved(plan if p is problems[0] else dataclasses.replace(plan, mu0=p.plan.mu0, mu1=p.plan.mu1), ms)
    return out


def bench_many(problems, reps=20):
    """Device-timed batched sweeps alone (dots_bench_many): milliseconds per batched solve of all the problems."""
    problems, hs = _handles(problems)
    ms = C.c_double()
    _lib.check(problems[0].lib.dots_bench_many(hs, len(problems), int(reps), C.byref(ms)), "dots_bench_many")
    return ms.value



_barycenter_scratch = {}      # (device ordinal, V) -> the scratch tensor of dots_barycenter_update


def barycenter_update(potentials, weights, eta, mass, nu, nu_device_order=None, vertex_row=None):
    """One mirror-descent step of a barycentre on the device (dots_barycenter_update, which takes no context;
    ``barycenter.update_host`` is the specification): ``nu`` (V,), a contiguous float64 tensor on a GPU, is updated in place from the
    ``potentials`` -- a list of 1 to 16 such tensors, ``phi0`` of each problem as ``sensitivity(to_device=True)`` left it --,
    ``weights``, ``eta`` and the total ``mass``, on torch's current stream of that device.  ``nu_device_order``: None, or a tensor that
    receives ``nu_device_order[vertex_row[v]] = nu[v]``; ``vertex_row``: an int32 tensor (V,) on the device, or None (the identity).
    Returns ``({"sum", "change", "gmax", "min"}, device milliseconds of the launches)``."""
    import torch

    if not isinstance(nu, torch.Tensor) or not nu.is_cuda or nu.ndim != 1:
        raise ValueError("barycenter_update: nu must be a float64 tensor of shape (V,) on a GPU")
    where, V = nu.device, int(nu.shape[0])
    for a in list(potentials) + [nu] + ([] if nu_device_order is None else [nu_device_order]):
        if not isinstance(a, torch.Tensor) or a.device != where or a.dtype != torch.float64 or tuple(a.shape) != (V,) or not a.is_contiguous():
            raise ValueError(f"barycenter_update: potentials, nu and nu_device_order must be contiguous float64 tensors of shape ({V},) on {where}")
    if vertex_row is not None and (not isinstance(vertex_row, torch.Tensor) or vertex_row.device != where or vertex_row.dtype != torch.int32
                                   or tuple(vertex_row.shape) != (V,) or not vertex_row.is_contiguous()):
        raise ValueError(f"barycenter_update: vertex_row must be a contiguous int32 tensor of shape ({V},) on {where}")
    n = len(potentials)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError(f"barycenter_update: weights must have shape ({n},), got {w.shape}")
    lib = _lib.load()
    key = (where.index, V)
    if key not in _barycenter_scratch:
        _barycenter_scratch[key] = torch.empty(int(lib.dots_barycenter_scratch(V)), dtype=torch.float64, device=where)
    pointers = (C.c_void_p * max(n, 1))(*[a.data_ptr() for a in potentials])
    scalars, ms = np.empty(4), C.c_double()
    d = _lib.BarycenterDesc()
    d.n, d.device, d.n_vertices = n, where.index, V
    d.phi0, d.weights = pointers, _ptr(w, C.c_double)
    d.eta, d.mass = float(eta), float(mass)
    d.nu, d.nu_device_order = nu.data_ptr(), None if nu_device_order is None else nu_device_order.data_ptr()
    d.vertex_row = None if vertex_row is None or nu_device_order is None else vertex_row.data_ptr()
    d.scratch, d.stream = _barycenter_scratch[key].data_ptr(), torch.cuda.current_stream(where).cuda_stream
    d.scalars, d.ms = _ptr(scalars, C.c_double), C.pointer(ms)
    _lib.check(lib.dots_barycenter_update(C.byref(d)), "dots_barycenter_update")
    return {"sum": float(scalars[0]), "change": float(scalars[1]), "gmax": float(scalars[2]), "min": float(scalars[3])}, ms.value


# ---- linearised transport (dots_tangent_*: calls without a context; dots_socp_amd.tangent holds the specifications) -----------------
def caller_tables(plan):
    """``{"triangles" (F, 3) int32, "hat" (F, 3, 3), "area" (F,), "mass" (V,)}``: the mesh tables of ``plan`` -- the ones a context
    built from it holds, in the device numbering -- in the CALLER's numbering, on the host; nothing is recomputed."""
    tri = np.asarray(plan.triangles, dtype=np.int32).reshape(-1, 3)
    hat = np.asarray(plan.hat_grad, dtype=np.float64).reshape(-1, 3, 3)
    area, mass = np.asarray(plan.area_tri, dtype=np.float64), np.asarray(plan.mass_vert, dtype=np.float64)
    if plan.perm_vert is not None:      # device vertex i is caller vertex perm_vert[i]; device triangle i is caller triangle perm_tri[i]
        pv, pf = np.asarray(plan.perm_vert, dtype=np.int64), np.asarray(plan.perm_tri, dtype=np.int64)
        t, h, a, m = np.empty_like(tri), np.empty_like(hat), np.empty_like(area), np.empty_like(mass)
        t[pf], h[pf], a[pf], m[pv] = pv[tri].astype(np.int32), hat, area, mass
        tri, hat, area, mass = t, h, a, m
    c = np.ascontiguousarray
    return {"triangles": c(tri), "hat": c(hat), "area": c(area), "mass": c(mass)}


def _tangent_desc(who, mesh, need):
    """The descriptor of a ``tangent_*`` call from the mesh tensors ``need`` names, its ``ms`` and the device"""
    import torch

    shapes = {"triangles": (torch.int32, lambda V, F: (F, 3)), "hat": (torch.float64, lambda V, F: (F, 3, 3)),
              "area": (torch.float64, lambda V, F: (F,)), "mass": (torch.float64, lambda V, F: (V,))}
    if not isinstance(mesh, dict) or any(not isinstance(mesh.get(k), torch.Tensor) or not mesh[k].is_cuda for k in need):
        raise ValueError(f"{who}: mesh must hold tensors on a GPU under {list(need)} (DeviceProblem.tangent_mesh)")
    where = mesh[need[0]].device
    V, F = int(mesh["mass"].shape[0]), int(mesh["triangles"].shape[0])      # (both calls need these two tables)
    for k in need:
        a, (dtype, shape) = mesh[k], shapes[k]
        if a.device != where or a.dtype != dtype or not a.is_contiguous() or tuple(a.shape) != shape(V, F):
            raise ValueError(f"{who}: mesh['{k}'] must be a contiguous {dtype} tensor of shape {shape('V', 'F')} on {where}")
    ms = C.c_double()
    d = _lib.TangentDesc()
    d.device, d.n_vertices, d.n_triangles = where.index, V, F
    d.triangles, d.hat_grad = mesh["triangles"].data_ptr(), mesh["hat"].data_ptr() if "hat" in need else None
    d.area_tri = mesh["area"].data_ptr() if "area" in need else None
    d.mass_vert = mesh["mass"].data_ptr() if "mass" in need else None
    d.stream, d.ms = torch.cuda.current_stream(where).cuda_stream, C.pointer(ms)
    return d, ms, where, V, F


def _tangent_tensor(who, name, a, where, shape):
    import torch

    if not isinstance(a, torch.Tensor) or a.device != where or a.dtype != torch.float64 or not a.is_contiguous() or (shape is not None and tuple(a.shape) != shape):
        raise ValueError(f"{who}: {name} must be a contiguous float64 tensor" + ("" if shape is None else f" of shape {shape}") + f" on {where}")


def tangent_velocities(mesh, potentials):
    """``(velocities, device milliseconds)``: ``velocities`` (n, F, 3), a new tensor on the device, the gradient of every potential on
    every triangle (dots_tangent_velocities; ``tangent.velocities_host`` is the specification, bit for bit).  ``mesh``: the tensors of
    ``DeviceProblem.tangent_mesh`` (caller's numbering); ``potentials``: a list of n >= 1 contiguous float64 tensors (V,) on that
    device, or one such tensor (n, V).  Needs n F 3 doubles of device memory.  On torch's current stream of that device."""
    import torch

    who = "tangent_velocities"
    d, ms, where, V, F = _tangent_desc(who, mesh, ("triangles", "hat", "mass"))
    rows = list(potentials)
    if not rows:
        raise ValueError(f"{who}: no potentials")
    for a in rows:
        _tangent_tensor(who, "every potential", a, where, (V,))
    out = torch.empty((len(rows), F, 3), dtype=torch.float64, device=where)
    pointers = (C.c_void_p * len(rows))(*[a.data_ptr() for a in rows])
    _lib.check(_lib.load().dots_tangent_velocities(C.byref(d), len(rows), pointers, out.data_ptr()), "dots_tangent_velocities")
    return out, ms.value


def tangent_weights(mesh, sigma):
    """``(w, device milliseconds)``: ``w`` (F,), a new tensor on the device, the mass of ``sigma`` (V,) on every triangle
    (dots_tangent_weights; ``tangent.weights_host`` is the specification, bit for bit)."""
    import torch

    who = "tangent_weights"
    d, ms, where, V, F = _tangent_desc(who, mesh, ("triangles", "area", "mass"))
    _tangent_tensor(who, "sigma", sigma, where, (V,))
    out = torch.empty((F,), dtype=torch.float64, device=where)
    _lib.check(_lib.load().dots_tangent_weights(C.byref(d), sigma.data_ptr(), out.data_ptr()), "dots_tangent_weights")
    return out, ms.value


_tangent_scratch = {}      # (device ordinal) -> the largest scratch tensor a Gram call has needed


def tangent_gram(A, B, w):
    """``(G, device milliseconds)``: ``G`` (na, nb), a host array, ``G[i][j] = sum_f w[f] A[i][f] . B[j][f]`` (dots_tangent_gram;
    ``tangent.gram_host`` is the specification: equal to an ulp, the same from call to call, symmetric bit for bit when ``B`` is
    None).  ``A`` (na, F, 3), ``B`` (nb, F, 3) or None (``A``), ``w`` (F,): contiguous float64 tensors on one GPU; na, nb <= 4096."""
    import torch

    who = "tangent_gram"
    if not isinstance(A, torch.Tensor) or not A.is_cuda or A.ndim != 3 or A.shape[2] != 3 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError(f"{who}: A must be a float64 tensor of shape (na, F, 3) on a GPU")
    where, na, F = A.device, int(A.shape[0]), int(A.shape[1])
    _tangent_tensor(who, "A", A, where, None)
    if B is not None:
        _tangent_tensor(who, "B", B, where, None)
        if B.ndim != 3 or B.shape[0] < 1 or tuple(B.shape[1:]) != (F, 3):
            raise ValueError(f"{who}: B must have shape (nb, {F}, 3), got {tuple(B.shape)}")
    _tangent_tensor(who, "w", w, where, (F,))
    nb = na if B is None else int(B.shape[0])
    lib = _lib.load()
    need = int(lib.dots_tangent_gram_scratch(na, nb, F))
    if need < 0:
        raise ValueError(f"{who}: na and nb must be 1 .. 4096, got {na} and {nb}")
    if where.index not in _tangent_scratch or _tangent_scratch[where.index].shape[0] < need:
        _tangent_scratch[where.index] = torch.empty(need, dtype=torch.float64, device=where)
    ms = C.c_double()
    d = _lib.TangentDesc()
    d.device, d.n_vertices, d.n_triangles = where.index, 1, F      # (the Gram call reads no vertex array)
    d.stream, d.ms = torch.cuda.current_stream(where).cuda_stream, C.pointer(ms)
    G = np.empty((na, nb))
    _lib.check(lib.dots_tangent_gram(C.byref(d), na, A.data_ptr(), nb, None if B is None else B.data_ptr(), w.data_ptr(),
                                     _tangent_scratch[where.index].data_ptr(), _ptr(G, C.c_double)), "dots_tangent_gram")
    return G, ms.value
