"""Solver plug-ins with the reference's names (``dot_surface_socp/socp/__init__.py:6-11``).

``solver_raw``  SOCP solver + conversion to DOT units          (socp/solver_decorator.py:10-27, utils/type.py:48-65)
``solver``      ``solver_raw`` on the time-centred grid          (socp/solver_decorator.py:29-54)
``solver_raw_many`` / ``solver_many``   the same for several problems on one surface with one shared factor (solver_socp_many)
``solver_raw_cascade`` / ``solver_cascade``   the same through a coarse-to-fine cascade in time (solver_socp_cascade)
``solver_raw_mesh_cascade`` / ``solver_mesh_cascade``   the same through a coarse-to-fine cascade in space (solver_socp_mesh_cascade)
``solver_raw_spacetime_cascade`` / ``solver_spacetime_cascade``   the same through a cascade in space and time at once
                                                                  (solver_socp_spacetime_cascade)
``solver_raw_auto_cascade`` / ``solver_auto_cascade``   the same through a cascade in space whose coarse meshes are made of the ONE
                                                        geometry the plug-in receives (solver_socp_auto_cascade)

``SolveSession``   one live context and one factor for a sequence of problems on one surface whose end masses change:
                   ``with SolveSession(n_time, geometry, **options) as s: solution, hist = s.solve(mu0, mu1, warm=True)`` (dots_restart)

``barycenter``     the Wasserstein barycentre of several measures on one surface, iterated on the device over one ``BatchSession``:
                   ``socp.barycenter(n_time, geometry, measures, weights)`` (dots_barycenter_update; ``dots_socp_amd.barycenter``)

``tangent_embedding`` / ``distance_matrix``   linearised transport: N measures seen from one reference measure, the Gram matrix of
                   their initial velocities formed on the device: ``socp.tangent_embedding(n_time, geometry, reference, measures)``,
                   ``socp.distance_matrix(n_time, geometry, measures)`` (dots_tangent_*; ``dots_socp_amd.tangent``)

Both take ``(n_time, geometry, **kwargs)`` and return ``(solution, run_history)``; they can be
passed as ``solver=`` to the reference's ``run_dot_surface`` (interface.py:106-134).

``readout="device"`` (the default) forms what they return -- ``mu`` and ``E`` in DOT units, ``mu`` on its final grid -- on the
device (``dots_readout``): two arrays cross to the host instead of twelve, and ``run_history.solver_stats["readout"]`` holds the
layer sums of ``mu`` (``evaluate.mass_conservation_from_layers`` / ``negative_mass_from_layers``).  ``readout="host"`` downloads
the whole solution and converts it in numpy: the same values bit for bit, kept as the baseline of measurements.

``flow_map={"starts": "vertices"}`` (the keywords of ``AlmSolver.flow_map``; default None: nothing changes) adds ``solution["flow_map"]``,
the transport map of the solution traced on the device (``dots_flow_map``; ``dots_socp_amd.flow.flow_map_host`` is the
specification): where every start point ends up and, with ``trajectory``, where it is after every interval.  Not on time slabs.

``sensitivity=True`` (or the keywords of ``AlmSolver.sensitivity``; default None: nothing changes) adds ``solution["sensitivity"]``: the
potentials at the two ends, the gradients of the cost in mu0 / mu1 and the stress of the kinetic energy, reduced on the device
(``dots_sensitivity``; ``dots_socp_amd.sensitivity`` holds the specification and ``cost_gradients``).  Not on time slabs; the stress
not with congestion.
"""
import numpy as np

from ..sensitivity import check_sensitivity
from .solver_socp import (BatchSession, DeviceOrdered, SolveSession, barycenter, check_flow_map, distance_matrix, solver_socp, solver_socp_auto_cascade, solver_socp_cascade, solver_socp_many,
                          solver_socp_mesh_cascade, solver_socp_spacetime_cascade, tangent_embedding)

__all__ = ["solver_socp", "solver_raw", "solver", "solver_socp_many", "solver_raw_many", "solver_many", "SolveSession", "BatchSession",
           "barycenter", "DeviceOrdered", "tangent_embedding", "distance_matrix",
           "solver_socp_cascade", "solver_raw_cascade", "solver_cascade",
           "solver_socp_mesh_cascade", "solver_raw_mesh_cascade", "solver_mesh_cascade",
           "solver_socp_spacetime_cascade", "solver_raw_spacetime_cascade", "solver_spacetime_cascade",
           "solver_socp_auto_cascade", "solver_raw_auto_cascade", "solver_auto_cascade"]


def _socp_to_dot(solution_socp, geom):
    """translate_solution_socp_to_dot (utils/type.py:48-65): densities -> masses / fluxes."""
    area_v = np.asarray(geom["area_vertices"], dtype=np.float64)
    area_t = np.asarray(geom["area_triangles"], dtype=np.float64)
    out = {
        "mu": solution_socp["mu"] * (area_v[np.newaxis, :] / 3.0),
        "E": solution_socp["E"] * area_t[np.newaxis, :, np.newaxis],
    }
    if solution_socp.get("checkpoints"):
        out["checkpoints"] = _checkpoints_to_dot(solution_socp["checkpoints"], geom)
    return out


def _checkpoints_to_dot(checkpoints, geom):
    area_v = np.asarray(geom["area_vertices"], dtype=np.float64)
    area_t = np.asarray(geom["area_triangles"], dtype=np.float64)
    return [
        {
            "mu": cp["mu"] * (area_v[np.newaxis, :] / 3.0),
            "E": cp["E"] * area_t[np.newaxis, :, np.newaxis],
            "iteration": cp["iteration"], "time": cp["time"], "kkt": cp["kkt"],
        }
        for cp in checkpoints
    ]


def _geometry_with_areas(geometry):
    if "area_vertices" in geometry and "area_triangles" in geometry:
        return geometry
    from ..meshes import triangle_areas, vertex_areas

    g = dict(geometry)
    g["area_triangles"] = triangle_areas(g["vertices"], g["triangles"])
    g["area_vertices"] = vertex_areas(np.asarray(g["vertices"]).shape[0], g["triangles"], g["area_triangles"])
    return g


def _read_out_spec(readout, centred, kwargs=None):
    """The ``read_out`` a plug-in hands its solver; with the plug-in's keywords, ``flow_map`` is checked first -- before the library
    is loaded -- and refused together with ``time_slab``; so is ``sensitivity``."""
    if kwargs is not None:
        check_flow_map(kwargs.get("flow_map"), kwargs.get("time_slab"))
        check_sensitivity(kwargs.get("sensitivity"), kwargs.get("time_slab"), kwargs.get("congestion", 0.0))
    if readout not in ("device", "host"):
        raise ValueError("readout must be 'device' or 'host'")
    return {"dot_units": True, "centred": centred} if readout == "device" else None


def _from_device(solution, geom):
    """The plug-in's dict from a solution that was read out on the device: ``mu`` and ``E`` are final, the checkpoints (in the
    solver's units) are converted as ever."""
    out = {"mu": solution["mu"], "E": solution["E"]}
    if solution.get("checkpoints"):
        out["checkpoints"] = _checkpoints_to_dot(solution["checkpoints"], geom)
    return out


def _finish(solution, geometry, mu0, mu1, readout, centred):
    """What a plug-in returns from what its solver returned."""
    g = _geometry_with_areas(geometry)
    if readout == "device":
        solution_dot = _from_device(solution, g)
    else:
        solution_dot = _socp_to_dot(solution, g)
        if centred:
            _to_time_centered(solution_dot, mu0, mu1)
    if centred:
        for cp in solution_dot.get("checkpoints") or []:
            _to_time_centered(cp, mu0, mu1)
    if "flow_map" in solution:      # (positions and barycentric weights: no units to convert)
        solution_dot["flow_map"] = solution["flow_map"]
    if "sensitivity" in solution:   # (in the units of geometry's mu0 / mu1 and vertices already)
        solution_dot["sensitivity"] = solution["sensitivity"]
    return solution_dot


def _end_points(geometry):
    return np.asarray(geometry["mu0"], dtype=np.float64), np.asarray(geometry["mu1"], dtype=np.float64)


def _to_time_centered(solution_dot, mu0, mu1):
    mid = 0.5 * (solution_dot["mu"][:-1] + solution_dot["mu"][1:])
    solution_dot["mu"] = np.concatenate([mu0[None, :], mid, mu1[None, :]], axis=0)


def _finest(geometries, who):
    geometries = list(geometries)
    if not geometries:
        raise ValueError(f"{who}: at least two geometries")
    return geometries, geometries[-1]


def _plug_in(driver, name, centred, finest=False, who=None, doc=None):
    """The plug-in ``name`` of ``driver``: its solution in DOT units on the time-staggered grid, or ``centred``: with the density on the
    time-centred grid and mu0 / mu1 as end points.  ``finest``: the plug-in takes ``geometries`` (coarse to fine) and returns the
    solution on the last one; ``who``: the driver in the message where there is none."""
    def run(n_time, geometry, geom, readout, kwargs):
        mu0, mu1 = _end_points(geom) if centred else (None, None)
        solution_socp, run_history = driver(n_time, geometry, read_out=_read_out_spec(readout, centred, kwargs), **kwargs)
        return _finish(solution_socp, geom, mu0, mu1, readout, centred), run_history

    if finest:
        def plug_in(n_time, geometries, readout="device", **kwargs):
            return run(n_time, *_finest(geometries, who), readout, kwargs)
    else:
        def plug_in(n_time, geometry, readout="device", **kwargs):
            return run(n_time, geometry, geometry, readout, kwargs)
    plug_in.__name__, plug_in.__doc__ = name, doc
    return plug_in


solver_raw = _plug_in(solver_socp, "dot_solver_socp", False,
                      doc="Solve the DOT problem with the GPU SOCP solver; solution on the time-staggered grid.")
solver = _plug_in(solver_socp, "dot_solver_socp_center", True,
                  doc="``solver_raw`` with the density moved to the time-centred grid and mu0 / mu1 as end points.")
solver_raw_cascade = _plug_in(solver_socp_cascade, "dot_solver_socp_cascade", False,
                              doc="``solver_raw`` through the time cascade (``solver_socp_cascade``: ``levels``, ``level_tol`` and the keywords of "
                                  "``solver_socp``).")
solver_cascade = _plug_in(solver_socp_cascade, "dot_solver_socp_cascade_center", True,
                          doc="``solver`` through the time cascade: the density on the time-centred grid with mu0 / mu1 as end points.")
solver_raw_mesh_cascade = _plug_in(solver_socp_mesh_cascade, "dot_solver_socp_mesh_cascade", False, True, "solver_socp_mesh_cascade",
                                   doc="``solver_raw`` on the finest of ``geometries`` through the cascade in space (``solver_socp_mesh_cascade``: "
                                       "``level_tol`` and the keywords of ``solver_socp``).")
solver_mesh_cascade = _plug_in(solver_socp_mesh_cascade, "dot_solver_socp_mesh_cascade_center", True, True, "solver_socp_mesh_cascade",
                               doc="``solver`` on the finest of ``geometries`` through the cascade in space: the density on the time-centred grid "
                                   "with the finest level's mu0 / mu1 as end points.")
solver_raw_spacetime_cascade = _plug_in(solver_socp_spacetime_cascade, "dot_solver_socp_spacetime_cascade", False, True, "solver_socp_spacetime_cascade",
                                        doc="``solver_raw`` on the finest of ``geometries`` through the cascade in space and time "
                                            "(``solver_socp_spacetime_cascade``: ``levels``, ``level_tol`` and the keywords of ``solver_socp``).")
solver_spacetime_cascade = _plug_in(solver_socp_spacetime_cascade, "dot_solver_socp_spacetime_cascade_center", True, True, "solver_socp_spacetime_cascade",
                                    doc="``solver`` on the finest of ``geometries`` through the cascade in space and time: the density on the "
                                        "time-centred grid with the finest level's mu0 / mu1 as end points.")
solver_raw_auto_cascade = _plug_in(solver_socp_auto_cascade, "dot_solver_socp_auto_cascade", False,
                                   doc="``solver_raw`` through a cascade in space made of ``geometry`` alone (``solver_socp_auto_cascade``: "
                                       "``coarse_levels``, ``ratio``, ``locate``, ``spacetime``, ``levels``, ``level_tol`` and the keywords of "
                                       "``solver_socp``): the signature of ``solver_raw``, so it can be passed as ``solver=`` where one geometry is "
                                       "handed over.")
solver_auto_cascade = _plug_in(solver_socp_auto_cascade, "dot_solver_socp_auto_cascade_center", True,
                               doc="``solver`` through a cascade in space made of ``geometry`` alone: the density on the time-centred grid with "
                                   "mu0 / mu1 as end points.")


def solver_raw_many(n_time, geometry, problems, readout="device", **kwargs):
    """``solver_raw`` for several problems on one surface (``solver_socp_many``): a list of ``(solution, run_history)``."""
    results = solver_socp_many(n_time, geometry, problems, read_out=_read_out_spec(readout, False, kwargs), **kwargs)
    return [(_finish(sol, geometry, None, None, readout, False), hist) for sol, hist in results]


def solver_many(n_time, geometry, problems, readout="device", **kwargs):
    """``solver`` for several problems on one surface: each density on the time-centred grid with its own mu0 / mu1 as end points."""
    results = solver_socp_many(n_time, geometry, problems, read_out=_read_out_spec(readout, True, kwargs), **kwargs)
    out = []
    for p, (sol, hist) in zip(problems, results):
        mu0 = np.asarray(p.get("mu0", geometry.get("mu0")), dtype=np.float64)
        mu1 = np.asarray(p.get("mu1", geometry.get("mu1")), dtype=np.float64)
        out.append((_finish(sol, geometry, mu0, mu1, readout, True), hist))
    return out
