"""The device calls the four drivers over live contexts make -- solver_socp, solver_socp_many, SolveSession.solve and
BatchSession.solve_many -- on the recording stand-in of DeviceProblem, in order, and the ``solver_stats["batch"]`` / ``["session"]``
records they write: one fixed script (session_checks.driver_calls) against what it returned on the commit before the drivers shared
their intake, their slot loop and their admission.  Printed there by
    python -c "import sys; sys.path[:0] = ['tests', '.']; import session_checks as s; s.print_driver_calls()"
and pasted in below.  An entry of LOG: the call, the number of its device (the order of creation within a driver: a session's slot),
then the problem (the letter of its end masses) and cold / warm where the call has them; ``share_frontal``: the device and the owner;
``step_many``: the devices of one lockstep group; ``finalize``: device, problem, tau, nit, tol."""
import session_checks as sc

NOTE = "phase times of a batched iteration are the batch's, booked to each active member as 1/n of them (n = members in that iteration)"
LOG = [('driver', 'solver_socp'), ('create', 0, 'A'), ('setup_frontal', 0), ('step', 0), ('finalize', 0, 'A', 1.9, 9, 0.001), ('close', 0),
 ('driver', 'solver_socp_many'), ('create', 0, 'A'), ('setup_frontal', 0), ('create', 1, 'B'), ('share_frontal', 1, 0), ('step_many', (0, 1)),
 ('finalize', 1, 'B', 1.9, 1000, 0.0001), ('create', 2, 'C'), ('share_frontal', 2, 0), ('upload', 2), ('upload', 2), ('upload', 2), ('upload', 2),
 ('upload', 2), ('upload', 2), ('upload', 2), ('upload', 2), ('close', 1), ('step_many', (0, 2)), ('step_many', (0, 2)),
 ('finalize', 0, 'A', 1.9, 1000, 0.0001), ('finalize', 2, 'C', 1.7, 1000, 0.0001), ('create', 3, 'D'), ('share_frontal', 3, 0), ('create', 4, 'E'),
 ('share_frontal', 4, 0), ('close', 0), ('close', 2), ('step_many', (3, 4)), ('finalize', 4, 'E', 1.9, 11, 0.0001), ('close', 4), ('step_many', (3,)),
 ('finalize', 3, 'D', 1.9, 1000, 0.0001), ('close', 3), ('driver', 'SolveSession first'), ('create', 0, 'A'), ('setup_frontal', 0), ('step', 0),
 ('finalize', 0, 'A', 1.9, 9, 0.001), ('driver', 'SolveSession warm'), ('restart', 0, 'B', 'warm'), ('step', 0), ('finalize', 0, 'B', 1.9, 11, 0.001),
 ('driver', 'SolveSession vertices'), ('move_vertices', 0), ('restart', 0, 'C', 'warm'), ('step', 0), ('finalize', 0, 'C', 1.9, 11, 0.001),
 ('driver', 'SolveSession cold'), ('restart', 0, 'D', 'cold'), ('step', 0), ('finalize', 0, 'D', 1.9, 11, 0.001), ('close', 0),
 ('driver', 'BatchSession cold'), ('create', 0, 'A'), ('setup_frontal', 0), ('create', 1, 'B'), ('share_frontal', 1, 0), ('create', 2, 'C'),
 ('share_frontal', 2, 0), ('step_many', (0, 1)), ('step_many', (2,)), ('finalize', 0, 'A', 1.8, 1000, 0.0001), ('finalize', 2, 'C', 1.8, 11, 0.0001),
 ('restart', 0, 'D', 'cold'), ('step_many', (0, 1)), ('finalize', 0, 'D', 1.8, 1000, 0.0001), ('finalize', 1, 'B', 1.8, 1000, 0.0001),
 ('driver', 'BatchSession warm'), ('restart', 0, 'B', 'warm'), ('restart', 1, 'A', 'warm'), ('step_many', (0, 1)),
 ('finalize', 1, 'A', 1.8, 1000, 0.001), ('step_many', (0,)), ('finalize', 0, 'B', 1.8, 1000, 0.0001), ('driver', 'BatchSession vertices'),
 ('move_vertices_many', (0, 1, 2)), ('restart', 0, 'E', 'cold'), ('restart', 1, 'D', 'cold'), ('restart', 2, 'C', 'cold'), ('step_many', (0, 1)),
 ('step_many', (2,)), ('finalize', 1, 'D', 1.8, 1000, 0.0001), ('finalize', 2, 'C', 1.8, 1000, 0.0001), ('restart', 1, 'B', 'cold'),
 ('restart', 2, 'A', 'cold'), ('step_many', (0, 1)), ('step_many', (2,)), ('finalize', 0, 'E', 1.8, 1000, 0.0001),
 ('finalize', 1, 'B', 1.8, 1000, 0.0001), ('finalize', 2, 'A', 1.8, 1000, 0.0001), ('close', 0), ('close', 1), ('close', 2),
 ('driver', 'BatchSession first vertices'), ('create', 0, 'A'), ('setup_frontal', 0), ('create', 1, 'E'), ('share_frontal', 1, 0),
 ('step_many', (0, 1)), ('finalize', 0, 'A', 1.9, 1000, 0.0001), ('finalize', 1, 'E', 1.9, 1000, 0.0001), ('close', 0), ('close', 1),
 ('driver', 'end')]
STATS = [
    ('solver_socp', {}),
    ('solver_socp_many', {'batch': {'size': 5, 'index': 0, 'max_batch': 2, 'steps_time_note': NOTE}}),
    ('solver_socp_many', {'batch': {'size': 5, 'index': 1, 'max_batch': 2, 'steps_time_note': NOTE}}),
    ('solver_socp_many', {'batch': {'size': 5, 'index': 2, 'max_batch': 2, 'steps_time_note': NOTE}}),
    ('solver_socp_many', {'batch': {'size': 5, 'index': 3, 'max_batch': 2, 'steps_time_note': NOTE}}),
    ('solver_socp_many', {'batch': {'size': 5, 'index': 4, 'max_batch': 2, 'steps_time_note': NOTE}}),
    ('SolveSession first', {'session': {'index': 0, 'warm': False, 'restart_ms': None, 'setup_seconds': 't', 'setup_seconds_saved': 0.0, 'moved': False, 'move_ms': None}}),
    ('SolveSession warm', {'session': {'index': 1, 'warm': True, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': False, 'move_ms': None}}),
    ('SolveSession vertices', {'session': {'index': 2, 'warm': True, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': True, 'move_ms': (0.125, 0.25, 0.5)}}),
    ('SolveSession cold', {'session': {'index': 3, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': False, 'move_ms': None}}),
    ('BatchSession cold', {'batch': {'size': 4, 'index': 0, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 0, 'warm': False, 'restart_ms': None, 'setup_seconds': 't', 'setup_seconds_saved': 0.0, 'moved': False, 'move_ms': None}}),
    ('BatchSession cold', {'batch': {'size': 4, 'index': 1, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 1, 'warm': False, 'restart_ms': None, 'setup_seconds': 't', 'setup_seconds_saved': 0.0, 'moved': False, 'move_ms': None}}),
    ('BatchSession cold', {'batch': {'size': 4, 'index': 2, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 2, 'warm': False, 'restart_ms': None, 'setup_seconds': 't', 'setup_seconds_saved': 0.0, 'moved': False, 'move_ms': None}}),
    ('BatchSession cold', {'batch': {'size': 4, 'index': 3, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 3, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': False, 'move_ms': None}}),
    ('BatchSession warm', {'batch': {'size': 2, 'index': 0, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 4, 'warm': True, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': False, 'move_ms': None}}),
    ('BatchSession warm', {'batch': {'size': 2, 'index': 1, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 5, 'warm': True, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': False, 'move_ms': None}}),
    ('BatchSession vertices', {'batch': {'size': 5, 'index': 0, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 6, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': True, 'move_ms': (0.125, 0.25, 0.5)}}),
    ('BatchSession vertices', {'batch': {'size': 5, 'index': 1, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 7, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': True, 'move_ms': (0.125, 0.25, 0.5)}}),
    ('BatchSession vertices', {'batch': {'size': 5, 'index': 2, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 8, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': True, 'move_ms': (0.125, 0.25, 0.5)}}),
    ('BatchSession vertices', {'batch': {'size': 5, 'index': 3, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 9, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': True, 'move_ms': (0.125, 0.25, 0.5)}}),
    ('BatchSession vertices', {'batch': {'size': 5, 'index': 4, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 10, 'warm': False, 'restart_ms': 0.25, 'setup_seconds': 't', 'setup_seconds_saved': 't', 'moved': True, 'move_ms': (0.125, 0.25, 0.5)}}),
    ('BatchSession first vertices', {'batch': {'size': 2, 'index': 0, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 0, 'warm': False, 'restart_ms': None, 'setup_seconds': 't', 'setup_seconds_saved': 0.0, 'moved': True, 'move_ms': None}}),
    ('BatchSession first vertices', {'batch': {'size': 2, 'index': 1, 'max_batch': 2, 'steps_time_note': NOTE}, 'session': {'index': 1, 'warm': False, 'restart_ms': None, 'setup_seconds': 't', 'setup_seconds_saved': 0.0, 'moved': True, 'move_ms': None}}),
]


def test_the_four_drivers_make_the_recorded_device_calls_and_write_the_recorded_records(monkeypatch):
    log, stats = sc.driver_calls(monkeypatch.setattr)
    for at, (got, want) in enumerate(zip(log, LOG)):      # (the first difference with what led to it reads better than two long lists)
        assert got == want, (at, log[max(0, at - 6):at + 1])
    assert log == LOG
    assert stats == STATS
    assert repr(stats) == repr(STATS)      # (the order of the keys too)
