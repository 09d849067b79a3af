"""CPU tests of the host-side mirror of the reference interface (hss.transforms.FSST,
hss.moments): constructor / attribute parity, error behaviour, fork/pickle safety, and that the
product never computes on the CPU."""
import inspect
import pickle

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import FSST, synth, transforms

KAISER = synth.kaiser_window(128, 0.5)
NO_GPU = not torch.cuda.is_available()


def test_constructor_signature_matches_reference():
    # /root/reference/hss/transforms/synchrosqueeze.py:13-21
    params = list(inspect.signature(FSST.__init__).parameters)
    assert params[:7] == ["self", "fs", "window", "abs", "stack", "truncate_freq", "dtype"]
    sig = inspect.signature(FSST.__init__).parameters
    assert sig["abs"].default is False and sig["stack"].default is False
    assert sig["truncate_freq"].default is None and sig["dtype"].default is torch.float32
    tf = FSST(1000, KAISER, truncate_freq=(25, 200), stack=True)
    assert tf.fs == 1000 and tf.window is KAISER and tf.abs is False and tf.stack is True
    assert tf.truncate_freq == (25, 200) and tf.dtype is torch.float32
    assert transforms.__all__ == ["Resample", "FSST"] and callable(tf)      # hss/transforms/__init__.py:5-8


def test_band_geometry_on_host(built_lib):
    assert FSST(1000, KAISER, truncate_freq=(25, 200)).band() == (4, 22)
    assert FSST(1000, KAISER).band() == (0, 65)
    assert FSST(1000, KAISER, truncate_freq=(1, 2)).band()[1] == 0


def test_truncate_valueerror_contract(built_lib):
    with pytest.raises(ValueError, match="truncate_freq must be set"):     # synchrosqueeze.py:104-105
        FSST(1000, KAISER)._truncate_frequencies(torch.zeros(65, 3), torch.zeros(65))
    s, f = FSST(1000, KAISER, truncate_freq=(25, 200))._truncate_frequencies(
        torch.arange(65.0)[:, None].repeat(1, 3), torch.arange(65.0) * 7.8125)
    assert s.shape == (22, 3) and f[0] == 31.25 and f[-1] == 195.3125


def test_pickle_drops_device_handles(built_lib):
    tf = FSST(1000, KAISER, truncate_freq=(25, 200), stack=True)
    tf._plans[("fake",)] = object()
    tf2 = pickle.loads(pickle.dumps(tf))
    assert tf2._plans == {} and tf2.truncate_freq == (25, 200) and np.array_equal(tf2.window, KAISER)


@pytest.mark.skipif(not NO_GPU, reason="checks the no-device failure mode")
def test_no_cpu_fallback(built_lib):
    tf = FSST(1000, KAISER, truncate_freq=(25, 200), stack=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tf(torch.zeros(2000))
    with pytest.raises(RuntimeError, match="no CPU"):
        FSST(1000, KAISER, device="cpu").batch(torch.zeros(2, 100))


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from heart_sounds_segmentation_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_product_never_imports_oracle():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "heart_sounds_segmentation_amd")
    for dp, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dp, fn)).read()
                assert "import oracle" not in text and "from oracle" not in text, fn
                assert "hss_oracle" not in text, fn


def test_frame_signal_golden_contract():
    """Window set fed to the path (hss/utils/preprocess.py:40-56 semantics pinned by the fixture):
    L = floor((T-n)/stride) frames, or ONE frame x[:n] when L <= 0."""
    from heart_sounds_segmentation_amd import framing
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "frame_signal.npz"))
    for T in (35000, 35500, 4000, 3000, 2500, 2000, 1500):
        starts, lens = framing.frame_starts(T, 1000, 2000)
        assert np.array_equal(starts, g[f"T{T}__starts"]), T
        assert np.array_equal(lens, g[f"T{T}__lens"]), T
    x = torch.arange(35500, dtype=torch.float32)
    F = framing.frame_batch(x, 1000, 2000)
    assert F.shape == (33, 2000) and F[5, 0] == 5000 and F[32, -1] == 33999


def test_consumer_matches_reference_segmenter_golden():
    """tests/golden/segmenter.npz was produced by the reference's HeartSoundSegmenter
    (hss/model/segmenter.py:5-87): same state_dict keys load, same output."""
    import os
    from heart_sounds_segmentation_amd.consumer import SegmenterHead
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "segmenter.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd__")}
    head = SegmenterHead(44, 12, 3, h0=torch.from_numpy(g["h0"]), c0=torch.from_numpy(g["c0"]))
    missing, unexpected = head.load_state_dict(sd, strict=True), None
    head.eval()
    with torch.no_grad():
        y = head(torch.from_numpy(g["x"]))
    assert y.shape == (3, 40, 4)
    assert np.abs(y.numpy() - g["y"]).max() < 1e-5


def test_consumer_c4_size_matches_reference_pipeline(oracle_mod):
    """BASELINE config C4 at its real size on the CPU: tests/golden/segmenter_c4.npz holds the output of the
    reference's own pipeline (reference FSST wrapper over the oracle core -> HeartSoundSegmenter(44, batch 50,
    hidden 240), hss/model/segmenter.py:20-87, main.py:170,221).  The weights are replayed from the seed (checksum
    pinned); the features come from the oracle's C epilogue."""
    import os
    from heart_sounds_segmentation_amd import synth
    from heart_sounds_segmentation_amd.consumer import SegmenterHead
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "segmenter_c4.npz"))
    head = SegmenterHead.seeded_like_reference(int(g["seed"])).eval()
    assert head.checksum() == g["sha256"].tobytes(), "weight replay differs from the reference-made fixture"
    X = synth.pcg_windows(50, 2000, seed=int(g["window_seed"]))
    feats = oracle_mod.features(X, 1000, synth.kaiser_window(128, 0.5), (25, 200), "stack", nthreads=8)
    assert np.abs(feats[:, ::250, :] - g["feat_probe"]).max() < 5e-6          # the reference wrapper's features
    with torch.no_grad():
        y = head(torch.from_numpy(feats))
    assert y.shape == (50, 2000, 4)
    assert np.abs(y.numpy() - g["y"]).max() < 2e-4                              # log-probabilities, absolute


def test_csv_ingest_matches_pandas(built_lib, tmp_path):
    """ingest.load_file == the reference's _load_file recipe (heart_sounds.py:193-197) on a synthetic
    file of the corpus format."""
    import pandas as pd
    from heart_sounds_segmentation_amd import ingest, _lib
    rng = np.random.default_rng(5)
    T = 5000
    sig = rng.standard_normal(T) * 0.3
    lab = rng.integers(1, 5, T)
    path = tmp_path / "a0001"
    with open(str(path) + ".csv", "w") as fh:
        fh.write("Signals,Labels\n")
        for i, (s, l) in enumerate(zip(sig, lab)):
            fh.write(f"{float(s)!r},{int(l)}\n" if i % 2 else f"{float(s):.9e},{int(l)}\n")
    df = pd.read_csv(str(path) + ".csv", skiprows=1, names=["Signals", "Labels"])
    x_ref = torch.tensor(df.loc[:, "Signals"].to_numpy(), dtype=torch.float32)
    y_ref = torch.tensor(df.loc[:, "Labels"].to_numpy(), dtype=torch.int64)
    x, y = ingest.load_file(str(path))
    assert x.dtype == torch.float32 and y.dtype == torch.int64 and x.shape == (T,)
    assert torch.equal(x, x_ref) and torch.equal(y, y_ref)
    with pytest.raises(ValueError):
        ingest.parse_csv_bytes(b"Signals,Labels\n0.5;1\n")
    assert ingest.parse_csv_bytes(b"Signals,Labels\n")[0].numel() == 0
    x2, y2 = ingest.parse_csv_bytes(b"Signals,Labels\r\n1.5,2.0\r\n\r\n-2e-3,4\n")
    assert x2.tolist() == [1.5, -0.0020000000949949026] and y2.tolist() == [2, 4]


def test_graft_entry_build_runs():
    """The driver's "does it build" check: __graft_entry__.build() compiles the library and the oracle and verifies
    the ABI version against the header (a hard-coded number once broke it after an ABI bump)."""
    import __graft_entry__ as g
    g.build()


def test_corpus_builder_groups_recordings_like_the_reference_loop():
    """SURVEY section 8f row 1 on the CPU: corpus.build_features lays recordings back to back and hands ALL frames of a
    group to one FSST.frames call; with a transform stand-in that returns the frames themselves, the items must be exactly
    what the reference's loop yields (heart_sounds.py:155-169: skip < frame_len, frame_signal's L = floor((T-n)/stride)
    frames -- one fewer than fit --, a single frame x[:n] when L <= 0, labels y - 1 framed alike), whatever the group size,
    and a rank's share is a contiguous block of recordings."""
    from heart_sounds_segmentation_amd.corpus import build_features
    from heart_sounds_segmentation_amd.framing import frame_batch

    class Identity:                                        # duck-typed FSST: features = the frame, as a (n, 1) block
        calls = 0

        def frames(self, x, starts, n, out=None):
            Identity.calls += 1
            return torch.stack([x[int(s):int(s) + n] for s in starts]).unsqueeze(-1)

    rng = np.random.default_rng(4)
    lens = (35000, 2500, 1999, 12345, 4000, 2000, 3000)
    recs = [(torch.from_numpy(rng.standard_normal(L).astype(np.float32)), torch.from_numpy(rng.integers(1, 5, L))) for L in lens]
    want = []
    for x, y in recs:                                      # the reference loop, restated with the golden-pinned framing
        if x.shape[0] < 2000:
            continue
        for fx, fy in zip(frame_batch(x, 1000, 2000), frame_batch(y - 1, 1000, 2000)):
            want.append((fx, fy))
    assert len(want) == 33 + 1 + 10 + 2 + 1 + 1
    for wpl in (1, 40, 4096):
        Identity.calls = 0
        got = build_features(recs, Identity(), device="cpu", windows_per_launch=wpl)
        assert len(got) == len(want)
        assert Identity.calls == {1: 6, 40: 2, 4096: 1}[wpl]       # (groups close at >= wpl frames: 33+1+10 | 2+1+1)
        for (gx, gy), (wx, wy) in zip(got, want):
            assert torch.equal(gx[:, 0], wx) and torch.equal(gy, wy) and gy.dtype == torch.int64
    parts = [build_features(recs, Identity(), device="cpu", rank=r, world=3) for r in range(3)]
    flat = [it for p in parts for it in p]
    assert len(flat) == len(want) and all(torch.equal(a[0][:, 0], b[0]) for a, b in zip(flat, want))


def test_pack_recordings_equals_python_framing(built_lib):
    """hssfsst_pack_recordings (the corpus builder's host side, one native call per group of recordings): the staging
    buffer is the recordings back to back and the frame starts are those of frame_signal
    (/root/reference/hss/utils/preprocess.py:30-58 as restated by framing.frame_starts), for lengths at and around the
    frame boundaries; capacity errors are reported, not overrun."""
    import ctypes
    from heart_sounds_segmentation_amd.framing import frame_starts
    recs = [torch.randn(T) for T in (35500, 2000, 2999, 3000, 3001, 4001, 35000, 2000)]
    ptrs = np.asarray([x.data_ptr() for x in recs], dtype=np.uint64)
    lens = np.asarray([x.numel() for x in recs], dtype=np.int64)
    stage = torch.empty(int(lens.sum()))
    starts = torch.empty(256, dtype=torch.int64)
    vp = ctypes.c_void_p
    for threads in (1, 3, 0):
        stage.zero_()
        nf = built_lib.hssfsst_pack_recordings(vp(ptrs.ctypes.data), vp(lens.ctypes.data), len(recs), 1000, 2000, vp(stage.data_ptr()),
                                               stage.numel(), vp(starts.data_ptr()), starts.numel(), threads)
        want, base = [], 0
        for x in recs:
            want.append(frame_starts(x.numel(), 1000, 2000)[0] + base)
            base += x.numel()
        want = np.concatenate(want)
        assert nf == len(want) and np.array_equal(starts[:nf].numpy(), want)
        assert torch.equal(stage, torch.cat(recs))
    assert built_lib.hssfsst_pack_recordings(vp(ptrs.ctypes.data), vp(lens.ctypes.data), len(recs), 1000, 2000, vp(stage.data_ptr()),
                                             stage.numel() - 1, vp(starts.data_ptr()), starts.numel(), 1) < 0
    assert built_lib.hssfsst_pack_recordings(vp(ptrs.ctypes.data), vp(lens.ctypes.data), len(recs), 1000, 2000, vp(stage.data_ptr()),
                                             stage.numel(), vp(starts.data_ptr()), 10, 1) < 0


def test_shipped_code_object_keeps_the_fixed_registers(built_lib):
    """fsst_team16_kernel keeps its held images in v104..v127 through inline assembly and tells the register allocator to
    stay below (amdgpu_num_vgpr: fsst_team16.hpp).  Checked on the SHIPPED library (the code object inside libhssfsst.so,
    disassembled): at least two team kernels; inside them the only instructions that name a register >= v104 are the two accessors
    (v_pk_mul_f32 into a pair, v_pk_add_f32 out of one), one held pair per instruction, all twelve pairs used; no AGPR, no call,
    128 registers reserved.  (A compiler that stopped honouring the limit would silently corrupt features.)
    __graft_entry__.build() runs the same check."""
    import os
    import pytest
    from heart_sounds_segmentation_amd import _lib
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    out = _lib.check_code_object()
    assert out["kernels"] >= 2 and out["metadata_checked"] >= 2 and out["accessor_instructions"] >= 100, out


def test_every_kernel_is_compiled_into_one_code_object(built_lib):
    """No kernel is compiled twice: the SHIPPED library's code objects (one per translation unit that holds kernels) are read and
    every kernel symbol is defined in exactly one of them -- a template kernel instantiated from two units would be in two, and
    whichever copy the loader registers last would win.  137 kernels in all; per family the counts of _lib.kernel_resources, which
    itself refuses a symbol it meets twice."""
    import os
    from heart_sounds_segmentation_amd import _lib
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    units = _lib.kernel_units()
    twice = {k: v for k, v in units.items() if len(v) != 1}
    assert not twice, twice
    assert len(units) == 137
    assert {m: len(_lib.kernel_resources(m)) for m in ("fsst_", "seg_", "resample")} == {"fsst_": 85, "seg_": 39, "resample": 13}


def test_translation_units():
    """The library's units (csrc/*.hip) are the ones _lib.SOURCES builds.  What the ``#include "..."`` lines, followed through the
    headers (_lib.include_closure, the walk build() dates its objects by), can decide about kernels: host_common.hpp and
    fsst_plan.hpp, which the FSST units share, hold none; a header that holds a kernel that is no template is reached from exactly
    ONE unit (it would be defined in every unit that reaches it); and hssfsst.hip, which routes to the launchers' units, reaches no
    header with a kernel at all.  (A template kernel's header may be reached from several units -- the MFMA core's is, one unit per
    transform length; that no instantiation is compiled twice is checked on the built library:
    test_every_kernel_is_compiled_into_one_code_object.)  Compiles nothing."""
    import os
    import re
    from heart_sounds_segmentation_amd import _lib
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert units == sorted(os.path.basename(s) for s in _lib.SOURCES)
    assert all(os.path.dirname(s) == csrc for s in _lib.SOURCES) and len(set(_lib.SOURCES)) == len(_lib.SOURCES)

    def text(name):
        with open(os.path.join(csrc, name)) as fh:
            return fh.read()

    by_unit = {u: _lib.include_closure(u) for u in units}
    assert "__global__" not in text("host_common.hpp") and "__global__" not in text("fsst_plan.hpp")
    assert all("host_common.hpp" in by_unit[u] for u in units) and "fsst_plan.hpp" in by_unit["hssfsst.hip"]
    def kernels(name):
        """per ``__global__`` of the file: is it a template?  (a ``template <...>`` head, comments apart, directly in front of it)"""
        code = re.sub(r"//[^\n]*", "", text(name))
        return [m.group(1) is not None for m in re.finditer(r"(template\s*<[^;{}]*>\s*)?__global__", code)]

    for h in sorted(f for f in os.listdir(csrc) if f.endswith((".hpp", ".h", ".hip"))):
        ks = kernels(h)
        users = [u for u in units if h == u or h in by_unit[u]]
        if ks:
            assert users, f"{h} holds a kernel and no unit reaches it"
            assert "hssfsst.hip" not in users, f"{h} holds a kernel and hssfsst.hip reaches it"
        if not all(ks):
            assert len(users) == 1, f"{h} holds a kernel that is no template and is reached from {users}"
    assert kernels("fsst_mfma128.hpp") == [True] and kernels("fsst_team16.hpp") == [True] and False in kernels("fsst_kernels.hpp")


def test_lent_buffer_goes_back_when_the_last_view_dies():
    """The drop-in call's result is a tensor over a pinned pool buffer the library LENT (hssfsst_exec_pinned): the ctypes array the tensor is made of
    hands the buffer back from its ``__del__`` -- once, with the buffer's address, and only when the last view of the result is gone."""
    import ctypes
    import os

    from heart_sounds_segmentation_amd.transforms import synchrosqueeze as sq

    backing = np.arange(2000 * 44, dtype=np.float32)
    released = []

    class FakeL:
        @staticmethod
        def hssfsst_pinned_release(handle, ptr):
            released.append(ptr.value)
            return 0

    class FakePlan:
        handle = ctypes.c_void_p(1234)
        pid = os.getpid()
        _L = FakeL

    buf = sq._lent_type(backing.size).from_address(backing.ctypes.data)
    buf._plan = FakePlan
    y = torch.from_numpy(np.frombuffer(buf, dtype=np.float32).reshape(2000, 44))
    del buf
    assert y.shape == (2000, 44) and float(y[1, 0]) == 44.0 and released == []
    v = y[10:12]
    del y
    assert released == []                                # a view keeps the buffer on loan
    assert float(v[0, 1]) == 441.0
    del v
    assert released == [backing.ctypes.data]
    assert sq._lent_type(backing.size) is sq._lent_type(backing.size)      # one array type per result size


def test_launch_shapes_under_sanitizers(tmp_path):
    """csrc/fsst_launch_shape.hpp alone, in a program of its own (tests/native/launch_shape_check.cpp) built with
    -fsanitize=address,undefined.  The plan facts and the plain-kernel table against the if-ladder they replace, for nwin 128 /
    256 / 512, every band, stack and not, pairs on and off: the same instantiation, and a row for every MFMA plan.  The team
    kernel's geometry over groups 0 .. 130, batches around 16, 256 and 65535 x 16, 1 .. 304 CUs, four LDS budgets and four
    strides: the arithmetic that stood in launch_team16, and for every accepted geometry the conditions the kernel's progress
    argument names (powers of two, cpc T >= G, cpc <= WPB, whole blocks of four, grid <= CUs, teams <= batch, slots >= 2 lead + 2
    within the LDS, lead + 1 <= pslots).  Chunk patterns of 1 .. 4 200 groups cover every group once; ragged lists cut each signal
    as alone, by region.  The z-score rule, the any-length kernel's tile search and the 88 % rule against their inline forms."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "launch_shape_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "heart_sounds_segmentation_amd", "csrc"),
                        os.path.join(root, "tests", "native", "launch_shape_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "launch shape ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
