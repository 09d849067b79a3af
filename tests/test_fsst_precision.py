"""The FSST kernels held to float32's own error, per 64-column block (tests/fsst_precision_cases.py has the restatements, the
emulation, the metric and the case table).  The contract's gate stays tests/parity.py at 1e-4 of a signal's largest feature; this
file adds, for every kernel family,

    ratio_j = max|out - oracle| over block j / (2^-24 ||span_j||_2 max|w|)  <=  8 x R32,

R32 = the largest ratio_j that two float32 restatements with float64 rounding decisions reach on the same case, computed at test
time from the reference side only; z-scored output, whose statistics are global, is gated per signal at 8 x Rz the same way.

CPU study (no GPU; figures measured with these inputs, Kaiser(128, 0.5) unless stated; multiples of the case's R32, the gate is 8;
the full table is in profiles/fsst_precision.txt):

  * R32 itself: 50 .. 65 u on pcg windows by the direct product and 12 .. 16 u by the FFT (u = the block's unit above), 15 .. 17 and 5
    on noise, 3 on isolated impulses, 80 .. 116 at 512 and 1024 points; Rz is 5e-7 .. 8e-7.
  * the faithful split-f16 emulation: 0.2 .. 2.4 x on every canonical case input -- under half the gate.
  * D1 / D2 (lo half of the samples / of the constants lost): 100 .. 1400 x.  Under parity.check at 1e-4 their max error passes
    (6e-5 .. 1e-4) and the L2 clause decides, within a few per cent either way: 0.98e-4 .. 1.4e-4.  D1 passes on dyn[1] and on
    Hann pcg[0], D2 on Hann pcg[1]; on the other windows the L2 clause catches them by 3 .. 40 %.
  * D3 (lo constant of the centre tap lost): 0.3 .. 5.6 x on pcg, noise, dyn, offset -- INSIDE the new gate.  The centre tap is the
    one tap whose twiddle is +-1 for every row, and w[64] = 0.999996 scales to 8191.97: the hi half takes all but 3.8e-6 of it (the
    other taps' lo halves are 2.3e-4).  Its loss is 63 u of the centre sample whatever the input: visible only where float32 itself
    is small -- isolated impulses (canon_clicks: 21 x) -- or under a window whose centre is not so close to a power of two
    (canon_hann: 39 .. 194 x).  The lo constants of an ordinary tap (tap 31, "D3g" in the report) are 9 .. 63 x on every other
    input and 1280 x on impulses.  So the table has the rows canon_clicks and canon_hann.
  * D4 (one scale per signal): 1.5 x on the 80 dB input ``dyn`` -- inside the gate, R32 being the largest block ratio of the case --,
    9 x with the stretch 100 dB down, 74 x at 120 dB (``deep``, added to the table for this), 870 x at 140 dB; 0.2 .. 2.4 x on
    everything else.  The block metric sees it from 120 dB on; a gate relative to the signal's maximum never does (9e-7 at 120 dB).
  * D5 (unreduced float32 angle): 6 .. 8 x at N = 512 (not twice the gate), 14 x on pcg and 31 .. 37 x on noise at N = 1024; passes 1e-4
    everywhere.  The 1024-point row is one row per input for this: pooled with pcg, noise is 16 x.
  * D6 (float32 decisions for cells below 1e-4 of the maximum): moves NO cell under Kaiser(0.5) on pcg, noise or dyn (its sidelobes
    keep every cell of a frame within 1e-2 of the frame's largest); under a Hann window off-bin tones move 1400 cells, 92 .. 156 x,
    and pass 1e-4 (3.9e-5).

On an MI355X (same file, -m gpu): canonical kernels 0.02 .. 0.62 x R32 (1.4 .. 12 u), fsst_core128_kernel and fsst_core_kernel
0.09 .. 0.50 x, fsst_dft_kernel 0.33 .. 1.19 x (it is a direct product itself), z-scored paths 0.19 .. 0.51 x Rz, the rolling step
0.22 x; canon_hann's tones 5.5 x (255 u) -- the closest any row comes to the gate.  Read from that row's output: the same
1.6e-4 appears with opposite signs in rows 13 and 14 of one column (5e-4 rows from a tie in the oracle), and the other worst errors
equal, to a few per cent, single source cells of 1e-6 .. 2e-6 of the signal's largest feature: whole cells in another row than the
oracle's, and cells of about 1e-6 R, the size below which the kernels leave the decision to float32 by design (kTieFloor2,
fsst_mfma128.hpp "Rounding ties": "they cannot change a feature by 1e-4 of the largest feature wherever they land").  That floor
was set for the 1e-4 gate; one such cell is worth a few hundred u, so it is what this gate sees first, and it is inside it.  No row
needed another bound.

With HSS_PRECISION_REPORT=<path> every case appends its line there (profiles/fsst_precision.txt).  Nothing here reads the
reference tree."""
import os

import numpy as np
import pytest

from tests import fsst_precision_cases as pc
from tests import parity
from tests.fsst_precision_cases import CASES, CASE_BY_ID, MARGIN

CASE_IDS = [c["id"] for c in CASES]
CANONICAL_IDS = [c["id"] for c in CASES if pc.is_canonical(c)]

# ---- the reference side, computed once per (case, signal) and left unchanged -----------------------------------------------------
_REF = {}
_R = {}


def _band(case, oracle_mod):
    if case["band"] is None:
        return 0, case["nwin"] // 2 + 1
    return oracle_mod.band(case["nwin"], case["fs"], *case["band"])


def _form(case, S):
    """Features in the form the case's call returns them: abs -> the magnitude, else complex."""
    return np.abs(S) if case["call"] == "abs" else S


def reference(case, label, x, oracle_mod):
    """dict of one signal: ref (K, n) complex128 from the C oracle, hd, rws (float64 rows), klo, K, d32 / f32 (the two float32
    restatements, complex64)."""
    key = (case["nwin"], case.get("window"), case["fs"], case["band"], label, x.size)
    if key not in _REF:
        w = pc.window(case)
        klo, K = _band(case, oracle_mod)
        s, _, _, hd = oracle_mod.fsst(x, case["fs"], w, return_halfdist=True)
        rws = pc.rows(x, case["fs"], w)
        _REF[key] = dict(x=x, w=w, klo=klo, K=K, ref=s[klo:klo + K], hd=hd, rws=rws,
                         d32=pc.float32_direct(x, w, rws, klo, K), f32=pc.float32_fft(x, w, rws, klo, K))
    return _REF[key]


def _cols(case, S):
    """The case's columns of (K, n) features, and the first of them."""
    if "cols" in case:
        c0, nc = case["cols"]
        return S[:, c0:c0 + nc], c0
    return S, 0


def _blocks(case, r, S):
    out, c0 = _cols(case, _form(case, S))
    ref, _ = _cols(case, _form(case, r["ref"]))
    return pc.block_ratios(out, ref, r["x"], r["w"], r["hd"], col0=c0)


def case_r32(case, oracle_mod):
    """(R32, Rz) of a case: the largest block ratio (largest z ratio) of the two float32 restatements over all its signals."""
    if case["id"] not in _R:
        r32 = rz = 0.0
        for label, x in pc.case_signals(case):
            r = reference(case, label, x, oracle_mod)
            z64 = pc.zscore64(r["ref"])
            for S in (r["d32"], r["f32"]):
                r32 = max(r32, pc.worst(_blocks(case, r, S)[0])["ratio"])
                rz = max(rz, pc.z_ratio(pc.float32_zscore(S), z64, r["hd"]))
        _R[case["id"]] = (r32, rz)
    return _R[case["id"]]


def _report(line):
    path = os.environ.get("HSS_PRECISION_REPORT")
    if not path:
        return
    new = not os.path.exists(path)
    with open(path, "a") as fh:
        if new:
            fh.write("FSST kernels against float32's own error per 64-column block (tests/test_fsst_precision.py).  u = 2^-24 ||span||_2 max|w| of a\n"
                     "block; R32 / Rz: the float32 restatements' largest block ratio (in u) / largest z error (of max|z64|) on the case; a kernel's\n"
                     "figures are multiples of R32 (Rz), the gate is 8.  Study lines: the split-f16 emulation and the defects on the CPU, as\n"
                     "multiples of the case's R32, with the verdict of parity.check at 1e-4 (P passes, F fails).\n\n")
        fh.write(line + "\n")


# ---- CPU: the reference side ------------------------------------------------------------------------------------------------------
def test_case_table():
    """Every row that names a row of tests/launch_cases.py names one that exists and whose recorded kernel contains the row's own
    kernel text; ids are unique; the dyn stretch is samples 640 .. 1343 at 2000 samples; the shapes stay small."""
    from tests.launch_cases import LAUNCH_CASES
    recorded = {name: kernel for name, _, kernel in LAUNCH_CASES}
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    for c in CASES:
        if c["launch"] is not None:
            assert c["kernel"] in recorded[c["launch"]], c["id"]
        assert max(np.atleast_1d(c["n"])) <= 2064 and c["gate"] in ("block", "z")
    assert pc.dyn_stretch(2000) == (640, 1344) and pc.dyn_stretch(640) == (192, 448) and pc.dyn_stretch(704) == (256, 448)
    x, p = pc.signals("dyn", 2000), pc.synth.pcg_windows(2, 2000, seed=pc._SEED["dyn"] + 2000)
    assert np.array_equal(x[:, :640], p[:, :640]) and np.abs(x[:, 640:1344]).max() <= 1.0001e-4 and np.array_equal(x[:, 1344:], p[:, 1344:])
    a = pc.signals("amp", 2000).astype(np.float64)
    assert np.array_equal(a[0] * 2.0 ** 80, a[1])


@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows_and_float64_values_are_the_oracle(cid, oracle_mod):
    """``rows`` with float64 values squeezed on them equals the C oracle to 1e-12 of the signal's largest feature, on every case
    input.  (oracle.features(..., "raw") is that oracle cast to complex64 -- asserted bit for bit -- so the comparison to 1e-12 is
    made before the cast, with oracle.fsst.)"""
    case = CASE_BY_ID[cid]
    for label, x in pc.case_signals(case):
        r = reference(case, label, x, oracle_mod)
        mine = pc.squeeze(pc.stft64(x, r["w"]), r["rws"], r["klo"], r["K"])
        scale = np.abs(r["ref"]).max()
        assert scale > 0 and np.abs(mine - r["ref"]).max() <= 1e-12 * scale, (cid, label, np.abs(mine - r["ref"]).max() / scale)
        raw = oracle_mod.features(x[None], case["fs"], r["w"], case["band"], "raw")[0]
        assert np.array_equal(raw, r["ref"].astype(np.complex64)), (cid, label)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_fragile_columns_of_the_oracle(cid, oracle_mod):
    """The oracle alone, on every case input: at most two rounding-fragile columns per signal and no block left without a robust
    column (the seeds are chosen so)."""
    case = CASE_BY_ID[cid]
    for label, x in pc.case_signals(case):
        r = reference(case, label, x, oracle_mod)
        _, nfrag, empty = _blocks(case, r, r["ref"])
        assert int((r["hd"] < parity.FRAG_EPS).sum()) <= 2 and empty == 0, (cid, label, nfrag, empty)


def test_metric_on_known_errors():
    """block_ratios on errors put there by hand: one cell of block 3 off by 5 u of that block, a fragile column ignored and counted,
    real and imaginary parts apart, a silent block with an error is inf, without one 0."""
    rng = np.random.default_rng(3)
    n, N, K = 300, 128, 4
    x = rng.standard_normal(n)
    x[0:127] = 0.0                                             # block 0 reads samples 0 .. 126 only: u_0 = 0
    w = np.kaiser(N, 0.5) * 0.5
    ref = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    hd = np.full(n, 0.25)
    hd[200] = 1e-9
    lo, hi = pc.block_span(3, n, N)
    assert (lo, hi) == (128, 300) and pc.block_span(0, n, N) == (0, 127) and pc.block_span(1, 2000, N) == (0, 191)
    u3 = 2.0 ** -24 * np.linalg.norm(x[lo:hi]) * 0.5 * np.kaiser(N, 0.5).max()
    out = ref.copy()
    out[2, 230] += 5j * u3
    out[1, 200] += 1.0                                         # in the fragile column
    bl, nfrag, empty = pc.block_ratios(out, ref, x, w, hd)
    assert nfrag == 1 and empty == 0 and [b["block"] for b in bl] == [0, 1, 2, 3, 4]
    assert bl[0]["u"] == 0.0 and bl[0]["ratio"] == 0.0
    assert abs(bl[3]["ratio"] - 5.0) < 1e-9 and (bl[3]["row"], bl[3]["col"]) == (2, 230)
    assert all(b["ratio"] == 0.0 for b in bl if b["block"] != 3)
    out[0, 5] += 1.0
    assert pc.block_ratios(out, ref, x, w, hd)[0][0]["ratio"] == float("inf")
    part, _, _ = pc.block_ratios(out[:, 8:72], ref[:, 8:72], x, w, hd, col0=8)
    assert [b["block"] for b in part] == [0, 1]


# ---- CPU: the study ---------------------------------------------------------------------------------------------------------------
SPLIT = {"emu": {}, "D1": dict(drop_x2=True), "D2": dict(drop_c2=True), "D3": dict(drop_c2_tap=64), "D3g": dict(drop_c2_tap=31),
         "D4": dict(one_scale=True)}
_STUDY = {}


def study(case, oracle_mod):
    """{label: {variant: (multiple of the case's R32, worst block, passes parity.check, rel max, rel L2)}} for the variants that
    apply to the case: the split-f16 emulation and D1 .. D4 where the kernel is a canonical one (128 points), D5 from 512 points,
    D6 everywhere."""
    if case["id"] in _STUDY:
        return _STUDY[case["id"]]
    r32, _ = case_r32(case, oracle_mod)
    out = {}
    for label, x in pc.case_signals(case):
        r = reference(case, label, x, oracle_mod)
        res = {}

        def put(name, S):
            wb = pc.worst(_blocks(case, r, S)[0])
            res[name] = (wb["ratio"] / r32, wb["block"]) + pc.old_gate(S, r["ref"], r["hd"])
        if pc.is_canonical(case):
            for name, kw in SPLIT.items():
                put(name, pc.split_f16(x, r["w"], r["rws"], r["klo"], r["K"], **kw))
        if case["nwin"] >= 512:
            put("D5", pc.float32_direct(x, r["w"], r["rws"], r["klo"], r["K"], twiddle="unreduced"))
        rows6, moved = pc.rows_d6(x, case["fs"], r["w"], r["rws"], float(np.abs(r["ref"]).max()))
        put("D6", pc.float32_direct(x, r["w"], rows6, r["klo"], r["K"]))
        res["moved"] = moved
        out[label] = res
    _STUDY[case["id"]] = out
    for label, res in out.items():
        line = (f"study {case['id']:16s} R32 {r32:6.2f} u  {label:10s}" + "".join(f" {k} {v[0]:.1f}{'P' if v[2] else 'F'}" for k, v in res.items() if k != "moved")
                + f"  (D6 moved {res['moved']} cells)")
        print(line)
        _report(line)
    return out


@pytest.mark.parametrize("cid", CANONICAL_IDS)
def test_faithful_emulation_is_within_half_the_gate(cid, oracle_mod):
    """The split-f16 emulation with nothing dropped stays at or below 4 x R32 -- half the gate -- on every canonical case input."""
    case = CASE_BY_ID[cid]
    for label, res in study(case, oracle_mod).items():
        assert res["emu"][0] <= MARGIN / 2, (cid, label, res["emu"])


# defect -> (case, signal) where parity.check at 1e-4 passes it, and (case, signal) where it is at least twice the new gate
PASSES_OLD = {"D1": ("canon_2000", "dyn[1]"), "D2": ("canon_hann", "pcg[1]"), "D3": ("canon_2000", "pcg[0]"), "D4": ("canon_2000", "deep[0]"),
              "D5": ("n1024_noise", "noise[0]"), "D6": ("canon_hann", "tone[0]")}
FAILS_NEW = {"D1": ("canon_2000", "pcg[0]"), "D2": ("canon_2000", "pcg[0]"), "D3": ("canon_clicks", "clicks[0]"),
             "D4": ("canon_2000", "deep[0]"), "D5": ("n1024_noise", "noise[0]"), "D6": ("canon_hann", "tone[0]")}


@pytest.mark.parametrize("defect", ["D1", "D2", "D3", "D4", "D5", "D6"])
def test_defects(defect, oracle_mod):
    """Each defect passes the suite's gate (parity.check at 1e-4) on a named case input -- the gap -- and is at least twice the
    new gate (16 x the case's R32) on a named case input.  D3 is also twice the gate on every input of canon_hann; D4 stays inside
    the gate on everything but ``deep`` (plain pcg and the 80 dB input included); D6 moves no cell under Kaiser(0.5)."""
    cid, label = FAILS_NEW[defect]
    res = study(CASE_BY_ID[cid], oracle_mod)[label][defect]
    assert res[0] >= 2 * MARGIN, (defect, cid, label, res)
    cid, label = PASSES_OLD[defect]
    res = study(CASE_BY_ID[cid], oracle_mod)[label][defect]
    assert res[2], (defect, cid, label, res)
    if defect == "D3":
        hann = study(CASE_BY_ID["canon_hann"], oracle_mod)
        assert all(r["D3"][0] >= 2 * MARGIN and r["D3"][2] for r in hann.values()), hann
    if defect == "D4":
        big = study(CASE_BY_ID["canon_2000"], oracle_mod)
        for lab, r in big.items():
            if not lab.startswith("deep"):
                assert r["D4"][0] <= MARGIN, (lab, r["D4"])            # plain pcg, noise, 80 dB, amplitudes, offsets: inside the gate
            else:
                assert r["D4"][0] >= 2 * MARGIN and r["D4"][2], (lab, r["D4"])
    if defect == "D6":
        assert study(CASE_BY_ID[cid], oracle_mod)[label]["moved"] > 100
        assert all(r["moved"] == 0 for lab, r in study(CASE_BY_ID["canon_2000"], oracle_mod).items() if lab.startswith(("pcg", "noise", "dyn")))


@pytest.mark.parametrize("cid", ["n512_unnorm"])
def test_unreduced_angle_at_512_points(cid, oracle_mod):
    """D5 at N = 512 passes 1e-4 and is above float32 on every input, yet not twice the gate (6 .. 11 x): it takes 1024 points."""
    for label, res in study(CASE_BY_ID[cid], oracle_mod).items():
        assert res["D5"][2] and 2.0 <= res["D5"][0], (label, res["D5"])


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def _kernel_name(tf, mode=None):
    import ctypes
    from heart_sounds_segmentation_amd import _lib
    buf = ctypes.create_string_buffer(160)
    _lib.check(_lib.lib().hssfsst_plan_last_kernel(tf._plan(0, mode).handle, buf, len(buf)), "hssfsst_plan_last_kernel")
    return buf.value.decode()


def _assert_kernel(case, name):
    """last_kernel() holds the row's kernel text and, where the row names one, the string tests/launch_cases.py recorded."""
    from tests.launch_cases import LAUNCH_CASES
    assert case["kernel"] in name, (case["id"], name)
    if case["launch"] is not None:
        recorded = {n: k for n, _, k in LAUNCH_CASES}[case["launch"]]
        assert name.startswith(recorded + " ["), (case["id"], name, recorded)
    if case["id"] == "n512_unnorm":
        assert name.startswith("fsst_core128_kernel<32, 16,"), name


def _run(case, X):
    """The case's call on a (B, n) float32 batch -> ([ (K, n) complex or (n, 2K) z per signal ], last_kernel())."""
    import torch
    from heart_sounds_segmentation_amd import FSST, _lib
    call = case["call"]
    tf = FSST(case["fs"], pc.window(case), abs=call == "abs", stack=call in ("stack", "unnormalized", "ragged"), truncate_freq=case["band"])
    if call == "ragged":
        res = tf.ragged([torch.from_numpy(np.array(x)).cuda() for x in X])
        outs = [res[i].float().cpu().numpy() for i in range(len(X))]
        return outs, _kernel_name(tf)
    Xd = torch.from_numpy(np.array(X)).cuda()
    if call == "unnormalized":
        U = tf.unnormalized(Xd, cols=case.get("cols")).cpu().numpy()
        K = U.shape[2] // 2
        full = np.zeros((U.shape[0], K, X.shape[1]), dtype=np.complex64)
        c0 = case["cols"][0] if "cols" in case else 0
        full[:, :, c0:c0 + U.shape[1]] = (U[..., :K] + 1j * U[..., K:]).transpose(0, 2, 1)
        return list(full), _kernel_name(tf, _lib.MODE_STACK_UNNORM)
    if "zpath" in case:
        tf.set_zpath(case["zpath"])
    out = tf.batch(Xd).cpu().numpy()
    if call == "abs":
        out = out.transpose(0, 2, 1)
    return list(out), _kernel_name(tf)


def _describe(case, r, wb):
    """What to read from a block: its index, the worst cell's row and column, the error, the block's unit, |S| against the block's norm,
    the column's distance from a rounding tie."""
    ref = _cols(case, r["ref"])[0]
    c0 = case["cols"][0] if "cols" in case else 0
    v = abs(ref[wb["row"], wb["col"] - c0])
    return (f"block {wb['block']} row {r['klo'] + wb['row']} col {wb['col']}: e {wb['e']:.3e} u {wb['u']:.3e} |S| / (u 2^24) {v / (wb['u'] * 2.0 ** 24 + 1e-300):.2e} "
            f"halfdist {r['hd'][wb['col']]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_kernel_within_eight_times_float32(cid, oracle_mod, built_lib):
    """One row of the table: the kernel it names ran, and every block of every signal is within 8 x R32 of the float64 oracle
    (z-scored output: every signal within 8 x Rz)."""
    case = CASE_BY_ID[cid]
    r32, rz = case_r32(case, oracle_mod)
    bound = MARGIN * (r32 if case["gate"] == "block" else rz)
    assert np.isfinite(bound) and bound > 0
    worst, where, fragile, kernels, failures = 0.0, "-", 0, set(), []
    for name in case["inputs"]:
        if case["call"] == "ragged":
            X = [pc.signals(name, n, case["fs"])[0] for n in case["n"]]
            labels = [f"{name}/{n}" for n in case["n"]]
        else:
            X = pc.signals(name, case["n"], case["fs"])
            labels = [f"{name}[{b}]" for b in range(len(X))]
        outs, kernel = _run(case, X)
        kernels.add(kernel)
        _assert_kernel(case, kernel)
        for label, x, out in zip(labels, X, outs):
            r = reference(case, label, x, oracle_mod)
            fragile += int((r["hd"] < parity.FRAG_EPS).sum())
            if case["gate"] == "block":
                assert out.shape == r["ref"].shape, (cid, label, out.shape)
                blocks = _blocks(case, r, out)[0]
                wb = pc.worst(blocks)
                print(f"{cid} {label}: worst {wb['ratio'] / r32:.2f} x R32 ({wb['ratio']:.1f} u), {_describe(case, r, wb)}")
                if wb["ratio"] >= worst:
                    worst, where = wb["ratio"], f"{label} {_describe(case, r, wb)}"
                failures += [f"{label} {_describe(case, r, b)}" for b in blocks if not b["ratio"] <= bound]
            else:
                assert out.shape == (x.size, 2 * r["K"]) and out.dtype == np.float32, (cid, label, out.shape, out.dtype)
                ratio = pc.z_ratio(out, pc.zscore64(r["ref"]), r["hd"])
                print(f"{cid} {label}: z error {ratio:.2e} = {ratio / rz:.2f} x Rz")
                if ratio >= worst:
                    worst, where = ratio, label
                if not ratio <= bound:
                    failures.append(f"{label} {ratio:.3e}")
    base = r32 if case["gate"] == "block" else rz
    _report(f"{cid:16s} {'R32' if case['gate'] == 'block' else 'Rz '} {base:9.3e}  worst {worst / base:6.2f} x ({where})  fragile columns {fragile}  {' | '.join(sorted(kernels))}")
    assert not failures, (cid, bound, failures[:6])


@pytest.mark.gpu
def test_streaming_step_within_eight_times_float32(oracle_mod, built_lib):
    """The rolling step on the canonical shape of tests/stream_cases.py: the un-normalised columns tests/test_streaming.py extracts,
    those whose frames hold no zero history, block-gated against the oracle of the signal (blocks of the offline columns: the
    step's own tiles start elsewhere, so here the blocks are only a partition)."""
    from tests import stream_cases as sc
    from tests import test_streaming as ts
    scase = sc.CASE_BY_ID[pc.STREAM_CASE]
    case = dict(id="stream_" + scase["id"], nwin=scase["nwin"], fs=scase["fs"], band=scase["band"], call="stream", window=None)
    assert scase["window"] == sc.KAISER
    x = sc.signals(scase)
    outs, kernel, _ = ts._unnormalized(scase)
    assert "fsst_canon_kernel<4, 22, false>" in kernel, kernel
    stream = np.concatenate(outs, axis=1)
    T, L = scase["steps"] * scase["chunk"], sc.lookahead(scase["nwin"])
    chans = sc.oracle_channels(scase["channels"])
    refs = {c: reference(case, f"stream ch{c}", x[c], oracle_mod) for c in chans}
    r32 = max(pc.worst(pc.block_ratios(S[:, :T - L], r["ref"][:, :T - L], r["x"], r["w"], r["hd"])[0])["ratio"]
              for r in refs.values() for S in (r["d32"], r["f32"]))
    worst, where, fragile, failures = 0.0, "-", 0, []
    for c, r in refs.items():
        K = r["K"]
        got = (stream[c, L:, :K] + 1j * stream[c, L:, K:]).T               # stream column t is offline column t - L
        blocks = pc.block_ratios(got, r["ref"][:, :T - L], r["x"], r["w"], r["hd"])[0]
        fragile += int((r["hd"] < parity.FRAG_EPS).sum())
        wb = pc.worst(blocks)
        print(f"stream ch{c}: worst {wb['ratio'] / r32:.2f} x R32, block {wb['block']}")
        if wb["ratio"] >= worst:
            worst, where = wb["ratio"], f"ch{c} block {wb['block']} row {r['klo'] + wb['row']} col {wb['col']}"
        failures += [(c, b) for b in blocks if not b["ratio"] <= MARGIN * r32]
    _report(f"{case['id']:16s} R32 {r32:9.3e}  worst {worst / r32:6.2f} x ({where})  fragile columns {fragile}  {kernel}")
    assert not failures, failures[:6]
