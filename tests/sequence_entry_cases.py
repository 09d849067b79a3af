"""Bad calls of the five sequence-model entry points (include/hssfsst.h: hssfsst_decode_states, hssfsst_decode_durations,
hssfsst_posteriors, hssfsst_posteriors_durations, hssfsst_posteriors_durations_counts) as a matrix, with no import from the
package: every case ends before the library looks for a device, or has count == 0, so the status and the text of
hssfsst_last_error() are the same on any machine.  Device-side pointers are fake non-NULL addresses that are never
dereferenced; ``offsets`` and the host tables of the two decoders are real arrays.

The matrix holds what the five test_argument_errors_need_no_device tests cover and, next to it, calls with two faults at once:
which of them is reported is part of each entry's contract (its order of checks), and it is what a shared helper gets wrong.

``python -m tests.sequence_entry_cases [library]`` records (entry, case, code, message) of every case into
tests/golden/sequence_entry_errors.json; tests/test_sequence_entries.py replays the matrix against the built library."""
import ctypes
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_entry_errors.json")
NINF = -np.inf
FAKE = 4096                                              # 16-byte aligned, never dereferenced
ODD2, ODD4, ODD8 = 4098, 4100, 4104                      # aligned to 2, 4 and 8 bytes only
BIG = 1 << 40                                            # a workspace size nothing here exceeds

_POST_DUR = ("logp", "offsets", "count", "a_pi", "durations", "edge", "max_duration", "labels", "gamma", "onsets", "loglik", "score", "xi", "s0")
ORDER = {
    "decode_states": ("logp", "offsets", "count", "transitions", "initial", "states", "scores", "device", "stream"),
    "decode_durations": ("logp", "offsets", "count", "transitions", "initial", "durations", "edge", "max_duration", "states", "scores",
                         "workspace", "workspace_bytes", "device", "stream"),
    "posteriors": ("logp", "offsets", "count", "a_pi", "labels", "gamma", "loglik", "score", "xi", "gamma0", "work", "work_bytes", "device",
                   "stream"),
    "posteriors_durations": _POST_DUR + ("work", "work_bytes", "device", "stream"),
    "posteriors_durations_counts": _POST_DUR + ("counts", "work", "work_bytes", "device", "stream"),
}
HOST_TABLES = {"decode_states": ("transitions", "initial"), "decode_durations": ("transitions", "initial", "durations", "edge")}
SCALARS = ("count", "max_duration", "workspace_bytes", "work_bytes", "device")
OPTIONAL = ("scores", "labels", "score", "xi", "gamma0", "s0", "onsets", "stream")        # NULL by default


def cyclic():
    A = np.full((4, 4), NINF, dtype=np.float32)
    for i in range(4):
        A[i, i] = A[i, (i + 1) % 4] = 0.0
    return A


def _with(a, index, value):
    a = a.copy()
    a[index] = value
    return a


def bind(L):
    """The argument types of the five entries on a library loaded with ctypes.CDLL (the package's loader sets the same)."""
    vp, c_int, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    ip, fp = ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_float)
    L.hssfsst_decode_states.argtypes = [vp, ip, c_i64, fp, fp, vp, vp, c_int, vp]
    L.hssfsst_decode_durations.argtypes = [vp, ip, c_i64, fp, fp, fp, fp, c_int, vp, vp, vp, c_i64, c_int, vp]
    L.hssfsst_posteriors.argtypes = [vp, ip, c_i64, vp, vp, vp, vp, vp, vp, vp, vp, c_i64, c_int, vp]
    L.hssfsst_posteriors_durations.argtypes = [vp, ip, c_i64, vp, vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp, vp, c_i64, c_int, vp]
    L.hssfsst_posteriors_durations_counts.argtypes = [vp, ip, c_i64, vp, vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, c_i64, c_int, vp]
    for name in ORDER:
        getattr(L, "hssfsst_" + name).restype = c_int
    L.hssfsst_last_error.restype = ctypes.c_char_p
    return L


def limits(L):
    """{entry: the step limit of a recording} as the library states it."""
    c_int, c_i64, ref = ctypes.c_int, ctypes.c_int64, ctypes.byref
    a, b, c = c_i64(0), c_i64(0), c_i64(0)
    assert L.hssfsst_decode_info(None, ref(a)) == 0 and L.hssfsst_decode_durations_info(None, ref(b), None) == 0
    assert L.hssfsst_posteriors_info(None, ref(c), None, None) == 0
    d = c_i64(0)
    assert L.hssfsst_posteriors_durations_info(None, None, ref(d), None, None, None) == 0
    return {"decode_states": a.value, "decode_durations": b.value, "posteriors": c.value, "posteriors_durations": d.value,
            "posteriors_durations_counts": d.value}


def list_cases(mx):
    """Bad lists, alone and two faults at a time; the precedence is: offsets[0], the lowest index that does not increase anywhere
    in the list, the lowest recording over the step limit, the total."""
    total = (1 << 31) // mx                              # recordings of mx steps that make 2^31 steps in all
    return [
        ("offsets0_not_zero", dict(offsets=[2, 4])),
        ("equal_at_2", dict(offsets=[0, 5, 5])),
        ("decrease_at_2", dict(offsets=[0, 7, 3])),
        ("equal_at_2_of_3", dict(offsets=[0, 4, 4, 9])),
        ("limit_hit_then_offsets0", dict(offsets=[1, 1 + mx])),
        ("recording_1_over_limit", dict(offsets=[0, 3, 3 + mx + 1])),
        ("steps_in_all_2^31", dict(offsets=[i * mx for i in range(total + 1)])),
        ("two:offsets0_and_decrease", dict(offsets=[3, 2, 9])),
        ("two:offsets0_and_over_limit", dict(offsets=[1, mx + 5])),
        ("two:over_limit_at_0_and_equal_at_2", dict(offsets=[0, mx + 1, mx + 2, mx + 2])),
        ("two:over_limit_at_0_and_2", dict(offsets=[0, mx + 1, mx + 2, 2 * mx + 9])),
        ("two:decrease_at_1_and_3", dict(offsets=[0, 0, 4, 4])),
        ("two:over_limit_and_steps_in_all", dict(offsets=[i * mx for i in range(total)] + [total * mx + 1])),
        ("two:equal_at_end_and_steps_in_all", dict(offsets=[i * mx for i in range(total + 1)] + [total * mx])),
        ("two:negative_offsets0_and_decrease", dict(offsets=[-4, -6])),
    ]


def common_cases(mx, required, aligned, work, work_bytes):
    """What every entry checks: count, the NULL scan over ``required`` in its order, device, the alignment scan over
    ``aligned`` = ((name, an address that is misaligned for it), ...) in its order, the list.  ``mx``: the entry's step limit."""
    out = [("count_0", dict(offsets=[0], count=0)),
           ("count_negative", dict(count=-1)),
           ("device_negative", dict(device=-1)),
           ("two:count_negative_and_null_logp", dict(count=-1, logp=None)),
           ("two:device_negative_and_misaligned_logp", dict(device=-1, logp=ODD4)),
           ("two:null_logp_and_device_negative", dict(logp=None, device=-1)),
           ("count_0_offsets0_not_zero", dict(offsets=[7], count=0)),
           ("count_0_misaligned_logp", dict(offsets=[0], count=0, logp=ODD8))]
    out += [(f"null_{name}", {name: None}) for name in required]
    out += [(f"two:null_{a}_and_{b}", {a: None, b: None}) for a, b in zip(required, required[1:])]
    out.append((f"two:null_{required[-1]}_and_{required[0]}", {required[-1]: None, required[0]: None}))
    out += [(f"misaligned_{name}", dict({name: addr}, **({"labels": FAKE} if name == "score" else {}))) for name, addr in aligned]
    out += [(f"two:misaligned_{a[0]}_and_{b[0]}", dict({a[0]: a[1], b[0]: b[1]}, **({"labels": FAKE} if "score" in (a[0], b[0]) else {})))
            for a, b in zip(aligned, aligned[1:])]
    if len(aligned) > 1:
        out.append((f"two:misaligned_{aligned[-1][0]}_and_{aligned[0][0]}", {aligned[-1][0]: aligned[-1][1], aligned[0][0]: aligned[0][1]}))
    out += list_cases(mx)
    out += [("two:misaligned_logp_and_equal_at_2", dict(logp=ODD4, offsets=[0, 5, 5])),
            ("two:null_offsets_and_misaligned_logp", dict(offsets=None, logp=ODD4))]
    if work:
        out += [(f"two:misaligned_{work}_and_too_small", {work: ODD8, work_bytes: 0}),
                ("two:misaligned_logp_and_too_small", {"logp": ODD4, work_bytes: 0}),
                (f"{work}_too_small_by_far", {work_bytes: 0}),
                (f"{work_bytes}_negative", {work_bytes: -1}),
                ("two:equal_at_2_and_too_small", {"offsets": [0, 5, 5], work_bytes: 0}),
                ("two:over_limit_and_too_small", {"offsets": [0, 3, 3 + mx + 1], work_bytes: 0}),
                ("two:offsets0_and_too_small", {"offsets": [2, 4], work_bytes: 0}),
                # a list at its limits passes: the call goes on to the workspace check
                ("limit_hit_exactly_then_too_small", {"offsets": [0, mx], work_bytes: 0}),
                ("steps_in_all_2^31-1_then_too_small", {"offsets": [i * mx for i in range((1 << 31) // mx)] + [(1 << 31) - 1], work_bytes: 0})]
    return out


def model_cases(diagonal_read):
    """Bad (transitions, initial) of the two decoders.  Every case whose tables are acceptable carries a bad list as well, so that
    it ends there: the list's error then says that the tables passed."""
    A, pi = cyclic(), np.zeros(4, dtype=np.float32)
    bad_list = [0, 5, 5]
    only_diagonal = _with(A, (1, 2), NINF)               # row 1 keeps its diagonal only
    beyond = _with(A, (slice(None), slice(None)), -1e30)                                  # clamped to -32768, not forbidden
    nan_and_dead = _with(_with(A, (1, slice(None)), NINF), (3, 0), np.nan)
    out = [
        ("nan_transitions_2_3", dict(transitions=_with(A, (2, 3), np.nan))),
        ("nan_initial_1", dict(initial=_with(pi, 1, np.nan))),
        ("dead_row_1", dict(transitions=_with(A, (1, slice(None)), NINF))),
        ("initial_all_forbidden", dict(initial=np.full(4, NINF, dtype=np.float32))),
        ("row_1_diagonal_only", dict(transitions=only_diagonal, offsets=bad_list)),
        ("tables_beyond_the_clamp_pass", dict(transitions=beyond, initial=np.full(4, -1e30, dtype=np.float32), offsets=bad_list)),
        ("tables_plus_inf_pass", dict(transitions=np.full((4, 4), np.inf, dtype=np.float32), offsets=bad_list)),
        ("two:nan_transitions_first_of_two", dict(transitions=_with(_with(A, (3, 1), np.nan), (0, 2), np.nan))),
        ("two:nan_transitions_and_nan_initial", dict(transitions=_with(A, (3, 3), np.nan), initial=_with(pi, 0, np.nan))),
        ("two:nan_initial_and_dead_row", dict(transitions=_with(A, (0, slice(None)), NINF), initial=_with(pi, 3, np.nan))),
        ("two:nan_transitions_behind_dead_row", dict(transitions=nan_and_dead)),
        ("two:dead_rows_0_and_2", dict(transitions=_with(_with(A, (0, slice(None)), NINF), (2, slice(None)), NINF))),
        ("two:dead_row_and_initial_all_forbidden", dict(transitions=_with(A, (3, slice(None)), NINF), initial=np.full(4, NINF, dtype=np.float32))),
        ("two:nan_transitions_and_bad_list", dict(transitions=_with(A, (2, 3), np.nan), offsets=bad_list)),
        ("two:nan_initial_and_offsets0", dict(initial=_with(pi, 2, np.nan), offsets=[2, 4])),
        ("two:dead_row_and_over_limit", dict(transitions=_with(A, (1, slice(None)), NINF), offsets=[0, 3, (1 << 27) + 9])),
        ("two:initial_all_forbidden_and_bad_list", dict(initial=np.full(4, NINF, dtype=np.float32), offsets=bad_list)),
        ("two:misaligned_logp_and_nan_transitions", dict(logp=ODD4, transitions=_with(A, (0, 0), np.nan))),
        ("two:count_0_and_nan_transitions", dict(offsets=[0], count=0, transitions=_with(A, (0, 0), np.nan))),
    ]
    if not diagonal_read:
        out.append(("two:row_0_diagonal_only_and_initial_all_forbidden",
                    dict(transitions=_with(A, (0, 1), NINF), initial=np.full(4, NINF, dtype=np.float32))))
    return out


def duration_table_cases(D):
    """Bad (durations, edge) of hssfsst_decode_durations, which reads them on the host, D columns each."""
    dur = np.zeros((4, D), dtype=np.float32)
    A = cyclic()
    nand, dead = _with(dur, (3, 2), np.nan), _with(dur, (2, slice(None)), NINF)
    last_only = _with(_with(dur, (1, slice(None)), NINF), (1, D - 1), -1e30)              # one allowed duration, beyond the clamp
    return [
        ("nan_durations_3_2", dict(durations=nand)),
        ("nan_edge_3_2", dict(edge=nand)),
        ("dead_durations_row_2", dict(durations=dead)),
        ("dead_edge_row_2", dict(edge=dead)),
        ("row_1_last_duration_only_passes", dict(durations=last_only, edge=last_only, offsets=[0, 5, 5])),
        ("two:nan_durations_and_nan_edge", dict(durations=nand, edge=_with(dur, (0, 0), np.nan))),
        ("two:dead_durations_row_before_its_nan", dict(durations=_with(dead, (3, 0), np.nan))),
        ("two:nan_durations_behind_dead_row_of_the_same_row", dict(durations=_with(dead, (2, D - 1), np.nan))),
        ("two:dead_edge_and_nan_durations", dict(durations=nand, edge=dead)),
        ("two:dead_durations_and_dead_edge", dict(durations=_with(dur, (3, slice(None)), NINF), edge=_with(dur, (0, slice(None)), NINF))),
        ("two:nan_transitions_and_nan_durations", dict(transitions=_with(A, (1, 1), np.nan), durations=nand)),
        ("two:nan_durations_and_row_without_successor", dict(transitions=_with(A, (1, 2), NINF), durations=nand)),
        ("two:dead_edge_and_initial_all_forbidden", dict(edge=dead, initial=np.full(4, NINF, dtype=np.float32))),
        ("two:nan_edge_and_bad_list", dict(edge=nand, offsets=[0, 5, 5])),
        ("two:dead_durations_and_too_small", dict(durations=dead, workspace_bytes=0)),
        ("two:max_duration_0_and_nan_durations", dict(max_duration=0, durations=nand)),
        ("two:misaligned_workspace_and_nan_edge", dict(workspace=ODD8, edge=nand)),
    ]


def max_duration_cases(limit, work_bytes):
    return [("max_duration_0", dict(max_duration=0)), ("max_duration_negative", dict(max_duration=-3)),
            ("max_duration_over_limit", dict(max_duration=limit + 1)),
            ("two:max_duration_0_and_misaligned_logp", dict(max_duration=0, logp=ODD4)),
            ("two:max_duration_over_limit_and_bad_list", dict(max_duration=limit + 1, offsets=[0, 5, 5])),
            ("two:device_negative_and_max_duration_0", dict(device=-1, max_duration=0)),
            ("two:max_duration_0_and_too_small", {"max_duration": 0, work_bytes: 0})]


def matrix(steps):
    """[(entry, case, overrides of the entry's default call)], every (entry, case) once.  ``steps``: limits()."""
    out = []
    D = 4
    for entry, diagonal_read in (("decode_states", True), ("decode_durations", False)):
        durations = entry == "decode_durations"
        required = ("logp", "offsets", "transitions", "initial") + (("durations", "edge") if durations else ()) + ("states",) \
            + (("workspace",) if durations else ())
        aligned = (("logp", ODD4),) + ((("workspace", ODD8),) if durations else ())
        cases = common_cases(steps[entry], required, aligned, "workspace" if durations else None, "workspace_bytes") + model_cases(diagonal_read)
        if durations:
            need = 8 * (5 + 8 * D)
            cases += duration_table_cases(D) + max_duration_cases(2048, "workspace_bytes")
            cases += [("workspace_one_byte_short", dict(workspace_bytes=need - 1)),
                      ("count_0_workspace_short_of_the_tables", dict(offsets=[0], count=0, workspace_bytes=8 * 8 * D - 1)),
                      ("count_0_workspace_of_the_tables", dict(offsets=[0], count=0, workspace_bytes=8 * 8 * D))]
        out += [(entry, name, kw) for name, kw in cases]
    post_req = ("logp", "offsets", "a_pi", "gamma", "loglik", "work")
    post_al = (("logp", ODD4), ("gamma", ODD8), ("work", ODD8), ("a_pi", ODD2), ("loglik", ODD4), ("score", ODD4), ("xi", ODD4), ("gamma0", ODD4))
    dur_req = ("logp", "offsets", "a_pi", "durations", "edge", "gamma", "loglik", "work")
    dur_al = (("logp", ODD4), ("gamma", ODD8), ("onsets", ODD8), ("work", ODD8), ("a_pi", ODD2), ("durations", ODD2), ("edge", ODD2),
              ("loglik", ODD4), ("score", ODD4), ("xi", ODD4), ("s0", ODD4))
    for entry, required, aligned in (("posteriors", post_req, post_al), ("posteriors_durations", dur_req, dur_al),
                                     ("posteriors_durations_counts", dur_req + ("counts",), dur_al + (("counts", ODD4),))):
        cases = common_cases(steps[entry], required, aligned, "work", "work_bytes")
        cases += [("score_without_labels", dict(score=FAKE)),
                  ("two:score_without_labels_and_null_gamma", dict(score=FAKE, gamma=None)),
                  ("two:score_without_labels_and_device_negative", dict(score=FAKE, device=-1)),
                  ("two:score_without_labels_and_misaligned_score", dict(score=ODD4)),
                  ("work_one_byte_short", dict(work_bytes="need-1")),
                  ("two:misaligned_optionals_xi_first", dict(xi=ODD4, **{aligned[-1][0]: ODD4}))]
        if entry != "posteriors":
            cases += max_duration_cases(2048, "work_bytes")
        if entry == "posteriors_durations_counts":
            cases += [("two:null_counts_and_null_work", dict(counts=None, work=None)),
                      ("two:null_counts_and_null_loglik", dict(counts=None, loglik=None)),
                      ("two:null_counts_and_misaligned_logp", dict(counts=None, logp=ODD4))]
        out += [(entry, name, kw) for name, kw in cases]
    assert len({(e, c) for e, c, _ in out}) == len(out)
    return out


def _need(L, entry, steps, count, D):
    """The smallest workspace of the three posteriors entries, from the library's own *_info figures."""
    c_i64, ref = ctypes.c_int64, ctypes.byref
    per, rec, dur = c_i64(0), c_i64(0), c_i64(0)
    if entry == "posteriors":
        assert L.hssfsst_posteriors_info(None, None, ref(per), ref(rec)) == 0
    elif entry == "posteriors_durations":
        assert L.hssfsst_posteriors_durations_info(None, None, None, ref(per), ref(rec), ref(dur)) == 0
    else:
        assert L.hssfsst_posteriors_durations_counts_info(ref(per), ref(rec), ref(dur), None) == 0
    return per.value * steps + rec.value * count + dur.value * D


def call(L, entry, overrides):
    """One call of ``entry`` with its defaults (a good call of one recording of 5 steps, D = 4 or 7) and ``overrides`` ->
    (status, the text of hssfsst_last_error(), "" for status 0)."""
    host = HOST_TABLES.get(entry, ())
    D = 4 if entry == "decode_durations" else 7
    kw = {name: (None if name in OPTIONAL else FAKE) for name in ORDER[entry]}
    kw.update(offsets=[0, 5], device=0, max_duration=D, workspace_bytes=BIG, work_bytes=BIG)
    if host:
        kw.update(transitions=cyclic(), initial=np.zeros(4, dtype=np.float32))
        kw.update(durations=np.zeros((4, D), dtype=np.float32), edge=np.zeros((4, D), dtype=np.float32))
    kw.update(overrides)
    if "count" not in overrides:
        kw["count"] = len(kw["offsets"]) - 1 if kw["offsets"] is not None else 1
    if kw["work_bytes"] == "need-1":
        kw["work_bytes"] = _need(L, entry, kw["offsets"][-1], kw["count"], D) - 1
    keep, args = [], []
    for name in ORDER[entry]:
        v = kw[name]
        if name in SCALARS:
            args.append(int(v))
        elif v is None:
            args.append(None)
        elif name == "offsets":
            keep.append((ctypes.c_int64 * len(v))(*v))
            args.append(keep[-1])
        elif name in host:
            keep.append(np.ascontiguousarray(v, dtype=np.float32))
            args.append(keep[-1].ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        else:
            args.append(ctypes.c_void_p(int(v)))
    rc = getattr(L, "hssfsst_" + entry)(*args)
    return rc, ("" if rc == 0 else L.hssfsst_last_error().decode("utf-8"))


def run(L):
    """Every case of the matrix -> [{"entry", "case", "code", "message"}]."""
    out = []
    for entry, case, kw in matrix(limits(L)):
        rc, msg = call(L, entry, kw)
        out.append({"entry": entry, "case": case, "code": rc, "message": msg})
    return out


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "heart_sounds_segmentation_amd", "libhssfsst.so")
    records = run(bind(ctypes.CDLL(path)))
    with open(GOLDEN, "w") as fh:
        json.dump(records, fh, indent=1)
        fh.write("\n")
    print(f"{len(records)} records from {path} -> {GOLDEN}")
