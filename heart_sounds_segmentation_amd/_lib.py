"""ctypes loader of libhssfsst.so (C ABI: include/hssfsst.h).

The shared library is built in-tree by ``build()`` (hipcc --offload-arch=gfx950) and is the only
compute implementation of this package: if it is missing or fails to load, every entry point raises
-- there is no Python/CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libhssfsst.so")
# the library's translation units: the FSST plan and its routing, one unit per FSST kernel family (the MFMA core in four, by transform
# length: the longest compiles first), and one per other subsystem.  No kernel is compiled into two of them (kernel_units)
SOURCES = [os.path.join(_PKG, "csrc", f) for f in (
    "fsst_core128_n512.hip", "fsst_core128_n512_pairs.hip", "fsst_core128_n256.hip", "fsst_generic.hip", "fsst_team.hip",
    "fsst_core128_n128.hip", "hssfsst.hip", "resample.hip", "segmenter.hip", "sequence.hip", "host_io.hip")]
BUILD_DIR = os.path.join(_PKG, "build")
HEADER = os.path.join(os.path.dirname(_PKG), "include", "hssfsst.h")

MODE_RAW, MODE_ABS, MODE_STACK, MODE_STACK_UNNORM = 0, 1, 2, 3
E_INVAL, E_NODEVICE, E_UNSUPPORTED, E_NOMEM, E_HIP = -1, -2, -3, -4, -5
DTYPE_F32, DTYPE_F64, DTYPE_F16, DTYPE_BF16 = 0, 1, 2, 3
STITCH_PROB, STITCH_LOGP, STITCH_SELECT = 0, 1, 2

_lock = threading.Lock()
_lib = None
_fork_warned = False
hip_owner_pid = None     # pid of the process in which this package first touched HIP (inherited by forked children)


class Launch(ctypes.Structure):
    """``hssfsst_launch`` of include/hssfsst.h: the device and the stream a call is enqueued on."""
    _fields_ = [("device", ctypes.c_int), ("stream", ctypes.c_void_p)]


class ForkedAfterGpuInitError(RuntimeError):
    """A DataLoader worker forked after its parent initialised the GPU tried to use the transform (a RuntimeError, as the
    reference's dataset expects, but also logged at ERROR and warned once: see ``guard_fork``)."""


def guard_fork() -> None:
    """HIP cannot be used in a child forked AFTER the parent initialised it (the reference forks DataLoader workers,
    /root/reference/main.py:202-218).  Creating the plan lazily in the worker is fine -- that is the supported pattern;
    a worker forked from a parent that already ran a transform gets a RuntimeError here (the exception the reference's
    dataset catches, hss/datasets/heart_sounds.py:183) instead of undefined behaviour inside the driver."""
    global hip_owner_pid
    pid = os.getpid()

    def refuse(msg: str):
        global _fork_warned
        # The reference's dataset catches RuntimeError, prints it and returns None (heart_sounds.py:183): with
        # in_memory=False and num_workers > 0 every sample of such a worker becomes None and the failure surfaces later, in
        # collate_fn.  Say it once, loudly, where it happens.
        import logging
        import warnings
        if not _fork_warned:                               # once per process: with in_memory=False every sample of the worker gets here
            _fork_warned = True
            logging.getLogger("heart_sounds_segmentation_amd").error(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=3)
        raise ForkedAfterGpuInitError(msg)

    if hip_owner_pid is not None and hip_owner_pid != pid:
        refuse("FSST: the HIP runtime was initialised in the parent process before this worker was forked; "
               "create / first use the transform inside the worker (lazy plan), or start workers with "
               "multiprocessing_context='spawn'")
    try:
        import torch
        bad = torch.cuda._is_in_bad_fork()
    except (ImportError, AttributeError):
        bad = False
    if bad:
        refuse("FSST: torch initialised the GPU in the parent process before this worker was forked; "
               "use multiprocessing_context='spawn' or touch the GPU only inside the workers")
    hip_owner_pid = pid


def include_closure(unit: str) -> set:
    """The files of csrc/ that the unit (or header) ``unit`` reaches through its ``#include "..."`` lines, followed through the
    headers: names relative to csrc/, the unit itself not among them.  (../../include/hssfsst.h lies outside csrc/ and is not
    listed: every unit depends on it.)"""
    import re
    csrc = os.path.join(_PKG, "csrc")
    seen, todo = set(), [os.path.basename(unit)]
    while todo:
        with open(os.path.join(csrc, todo.pop())) as fh:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M):
                inc = os.path.normpath(inc)
                if inc not in seen and os.path.exists(os.path.join(csrc, inc)):
                    seen.add(inc)
                    todo.append(inc)
    return seen


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the units of SOURCES for gfx950, each into an object under build/, and link them into libhssfsst.so (cross-compiles
    without a GPU).  An object is rebuilt when it is older than its own unit, a header of csrc/ that the unit reaches
    (include_closure) or the C header; the units that need it compile concurrently.  A failed unit raises after the others have
    finished, and nothing is linked.  A library that is newer than every unit and every header they reach is current whether or not
    the objects are there (a copy of the tree without build/)."""
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.dirname(SOURCES[0])
    deps = {src: [src, HEADER] + sorted(os.path.join(csrc, h) for h in include_closure(src)) for src in SOURCES}
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def older(target: str, deps) -> bool:
        return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)

    def run(cmd) -> None:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if verbose or res.returncode != 0:
            print(res.stdout)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed ({res.returncode}): {' '.join(cmd)}\n{res.stdout}")

    if not force and not older(LIB_PATH, [d for src in SOURCES for d in deps[src]]):
        return LIB_PATH
    objects = [os.path.join(BUILD_DIR, os.path.splitext(os.path.basename(src))[0] + ".o") for src in SOURCES]
    stale = [(src, obj) for src, obj in zip(SOURCES, objects) if force or older(obj, deps[src])]
    if stale:
        os.makedirs(BUILD_DIR, exist_ok=True)
        jobs = min([len(SOURCES), 16] + ([max(int(os.environ["MAX_JOBS"]), 1)] if os.environ.get("MAX_JOBS", "").isdigit() else []))
        with ThreadPoolExecutor(max_workers=jobs) as pool:
            done = [pool.submit(run, [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o", obj, src])
                    for src, obj in stale]
        for d in done:                                     # (all of them have finished: the first failure is raised)
            d.result()
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objects)      # (it is missing, or older than an object)
    return LIB_PATH


def _llvm_tools(*names) -> dict:
    """Paths of the llvm tools that look into the built library; RuntimeError when one is missing."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = {t: (shutil.which(t) or os.path.join(llvm, t)) for t in names}
    tools["objcopy"] = shutil.which("objcopy") or shutil.which("llvm-objcopy") or os.path.join(llvm, "llvm-objcopy")
    for t in tools.values():
        if not os.path.exists(t):
            raise RuntimeError(f"check_code_object: {t} not found")
    return tools


def _unbundle(tools: dict, path: str, td: str) -> list:
    """The gfx950 code objects inside the library ``path``, written into the directory ``td``: one per translation unit.  The
    library's .hip_fatbin section holds the units' bundles back to back and the unbundler reads only the first of a file, so the
    section is cut at every bundle header."""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    fat = os.path.join(td, "fat.bin")
    subprocess.run([tools["objcopy"], "-O", "binary", "--only-section=.hip_fatbin", path, fat], check=True, capture_output=True)
    with open(fat, "rb") as f:
        data = f.read()
    cuts, at = [], data.find(magic)
    while at >= 0:
        cuts.append(at)
        at = data.find(magic, at + len(magic))
    cuts.append(len(data))
    objs = []
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        piece, obj = os.path.join(td, f"fat{k}.bin"), os.path.join(td, f"code{k}.o")
        with open(piece, "wb") as f:
            f.write(data[lo:hi])
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={piece}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={obj}"], check=True, capture_output=True)
        objs.append(obj)
    return objs


def kernel_resources(match: str, path: str = None) -> dict:
    """What the SHIPPED code object says of its kernels whose name contains ``match``: ``llvm-readelf --notes`` of the gfx950 code
    object inside the library -> {mangled name: {"vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size" (scratch
    bytes per lane), "group_segment_fixed_size" (LDS bytes)}}.  RuntimeError without the llvm tools."""
    import re
    import tempfile
    tools = _llvm_tools("clang-offload-bundler", "llvm-readelf")
    with tempfile.TemporaryDirectory() as td:
        notes = "".join(subprocess.run([tools["llvm-readelf"], "--notes", obj], check=True, capture_output=True, text=True).stdout
                        for obj in _unbundle(tools, path or LIB_PATH, td))
    out = {}
    fields = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or match not in name.group(1):
            continue
        if name.group(1) in out:                          # (compiled into two code objects: the loader registers both, the last one wins)
            raise RuntimeError(f"kernel_resources: {name.group(1)} is defined in two code objects")
        out[name.group(1)] = {f: int(re.search(r"\." + f + r":\s+(\d+)", blk).group(1)) for f in fields}
    return out


def kernel_units(path: str = None) -> dict:
    """Where the SHIPPED library's kernels are defined: {kernel symbol: [index of each code object -- one per translation unit that
    holds kernels -- whose metadata names it]}.  A kernel in two code objects was compiled twice (a template instantiated from two
    units); the loader registers both and the last one wins.  RuntimeError without the llvm tools."""
    import re
    import tempfile
    tools = _llvm_tools("clang-offload-bundler", "llvm-readelf")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for k, obj in enumerate(_unbundle(tools, path or LIB_PATH, td)):
            notes = subprocess.run([tools["llvm-readelf"], "--notes", obj], check=True, capture_output=True, text=True).stdout
            for name in re.findall(r"^\s*\.name:\s+(\S+)\s*$\n\s*\.private_segment_fixed_size:", notes, re.M):
                out.setdefault(name, []).append(k)
    return out


def check_code_object(path: str = None) -> dict:
    """The SHIPPED code object, looked at: fsst_team16_kernel keeps its held images in v104..v127 through inline assembly and compiles for 104
    allocatable registers (fsst_team16.hpp) -- a compiler that stopped honouring the limit, started using AGPRs or outlined a call would corrupt
    features silently.  Disassembles the gfx950 code object inside the library and asserts, for every team kernel: the only instructions
    that name a register >= v104 are the two accessors, all twelve pairs are used, no AGPR, no call, 128 registers reserved.  Returns counts."""
    import re
    import tempfile
    path = path or LIB_PATH
    tools = _llvm_tools("clang-offload-bundler", "llvm-objdump", "llvm-readelf")
    with tempfile.TemporaryDirectory() as td:
        dis, notes = [], ""
        for obj in _unbundle(tools, path, td):               # the unit whose code object holds the team kernels
            n = subprocess.run([tools["llvm-readelf"], "--notes", obj], check=True, capture_output=True, text=True).stdout
            if "fsst_team16_kernel" not in n:
                continue
            dis += subprocess.run([tools["llvm-objdump"], "-d", "--mcpu=gfx950", obj], check=True, capture_output=True, text=True).stdout.split("\n")
            notes += n
    starts = [i for i, ln in enumerate(dis) if re.match(r"^[0-9a-f]+ <_ZN7hssfsst18fsst_team16_kernel.*>:", ln)]
    if len(starts) < 2:
        raise RuntimeError("check_code_object: the team kernels are not in the code object")
    put = re.compile(r"^\s*v_pk_mul_f32 v\[(\d+):(\d+)\], v\[\d+:\d+\], v\[\d+:\d+\]\s*$")
    get = re.compile(r"^\s*v_pk_add_f32 v\[\d+:\d+\], v\[(\d+):(\d+)\], v\[\d+:\d+\] op_sel")
    out = {"kernels": 0, "accessor_instructions": 0}
    for st in starts:
        seen = set()
        for ln in dis[st + 1:]:
            if re.match(r"^[0-9a-f]+ <.*>:", ln):
                if "_ZN7hssfsst" in ln and "fsst_team16_kernel" not in ln:
                    break
                continue
            code = ln.split("//")[0]
            if re.search(r"\bs_swappc_b64\b|\bs_call_b64\b|\bs_setpc_b64\b", code):
                raise RuntimeError(f"check_code_object: a call inside the team kernel: {code.strip()}")
            if re.search(r"\ba\d+\b|\ba\[\d+:\d+\]|v_accvgpr", code):
                raise RuntimeError(f"check_code_object: an AGPR inside the team kernel: {code.strip()}")
            regs = [int(a) for a in re.findall(r"\bv(\d+)\b", code)] + [int(b) for _, b in re.findall(r"\bv\[(\d+):(\d+)\]", code)]
            if not regs or max(regs) < 104:
                continue
            m = put.match(code) or get.match(code)
            if not (m and int(m.group(1)) >= 104 and int(m.group(2)) == int(m.group(1)) + 1):
                raise RuntimeError(f"check_code_object: register >= v104 outside the accessors: {code.strip()}")
            if sum(1 for _, b in re.findall(r"\bv\[(\d+):(\d+)\]", code) if int(b) >= 104) != 1:
                raise RuntimeError(f"check_code_object: two held pairs in one instruction: {code.strip()}")
            seen.add(int(m.group(1)))
            out["accessor_instructions"] += 1
        if seen != set(range(104, 128, 2)):
            raise RuntimeError(f"check_code_object: held pairs used: {sorted(seen)}")
        out["kernels"] += 1
    # the kernels' metadata: 128 vector registers, no AGPR
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        if "fsst_team16_kernel" not in blk.split(".symbol:")[0] + blk:
            continue
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "fsst_team16_kernel" not in name.group(1):
            continue
        agpr = int(blk.strip().split()[0])
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        if agpr != 0 or not vg or int(vg.group(1)) != 128:
            raise RuntimeError(f"check_code_object: {name.group(1)}: agpr_count {agpr}, vgpr_count {vg.group(1) if vg else None}")
        out["metadata_checked"] = out.get("metadata_checked", 0) + 1
    if out.get("metadata_checked", 0) < 2:
        raise RuntimeError("check_code_object: the team kernels' metadata was not found")
    return out


def lib():
    """The loaded C-ABI library; raises RuntimeError when it is absent (no fallback)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is the only implementation of the FSST "
                "path (no CPU fallback). Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or heart_sounds_segmentation_amd._lib.build().")
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 not found
            raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
        c_int, c_dbl, c_i64 = ctypes.c_int, ctypes.c_double, ctypes.c_int64
        vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
        dp = ctypes.POINTER(ctypes.c_double)
        L.hssfsst_plan_create.argtypes = [ctypes.POINTER(vp), c_int, c_int, dp, c_dbl, c_int, c_dbl, c_dbl, c_int]
        L.hssfsst_plan_create.restype = c_int
        L.hssfsst_plan_create_ex.argtypes = [ctypes.POINTER(vp), c_int, c_int, dp, c_dbl, c_int, c_dbl, c_dbl, c_int, c_int]
        L.hssfsst_plan_create_ex.restype = c_int
        L.hssfsst_plan_out_dtype.argtypes = [vp, ip]
        L.hssfsst_plan_out_dtype.restype = c_int
        L.hssfsst_plan_destroy.argtypes = [vp]
        L.hssfsst_plan_destroy.restype = c_int
        L.hssfsst_plan_info.argtypes = [vp, ip, ip, ip, ip, ip, ip, ip]
        L.hssfsst_plan_info.restype = c_int
        L.hssfsst_exec.argtypes = [vp, vp, c_i64, c_int, c_int, vp, c_int, vp]
        L.hssfsst_exec.restype = c_int
        L.hssfsst_exec_cols.argtypes = [vp, vp, c_i64, c_int, c_int, c_int, c_int, vp, c_int, vp]
        L.hssfsst_exec_cols.restype = c_int
        L.hssfsst_exec_frames.argtypes = [vp, vp, c_i64, c_int, c_i64, c_int, c_int, c_int, vp, c_int, vp]
        L.hssfsst_exec_frames.restype = c_int
        L.hssfsst_exec_pinned.argtypes = [vp, vp, c_int, ctypes.POINTER(vp)]
        L.hssfsst_exec_pinned.restype = c_int
        L.hssfsst_pinned_release.argtypes = [vp, vp]
        L.hssfsst_pinned_release.restype = c_int
        L.hssfsst_normalize_running.argtypes = [vp, vp, c_i64, c_int, vp, vp]
        L.hssfsst_normalize_running.restype = c_int
        L.hssfsst_exec_list.argtypes = [vp, vp, c_i64, vp, c_int, c_i64, c_int, c_int, vp, c_int, vp]
        L.hssfsst_exec_list.restype = c_int
        L.hssfsst_exec_ragged.argtypes = [vp, vp, c_i64, vp, vp, c_i64, c_int, vp, c_int, vp]
        L.hssfsst_exec_ragged.restype = c_int
        L.hssfsst_stream_step.argtypes = [vp, vp, c_i64, c_i64, vp, c_i64, c_int, c_int, c_int, vp, vp, vp, vp]
        L.hssfsst_stream_step.restype = c_int
        L.hssfsst_plan_last_exec_fused.argtypes = [vp]
        L.hssfsst_plan_set_zpath.argtypes = [vp, c_int]
        L.hssfsst_plan_fallbacks.argtypes = [vp]
        L.hssfsst_allgather.argtypes = [vp, vp, c_i64, vp, vp, c_int]
        L.hssfsst_allgather.restype = c_int
        L.hssfsst_plan_last_kernel.argtypes = [vp, ctypes.c_char_p, c_int]
        L.hssfsst_plan_last_kernel.restype = c_int
        L.hssfsst_plan_fallbacks.restype = c_int
        L.hssfsst_plan_set_zpath.restype = c_int
        L.hssfsst_plan_last_exec_fused.restype = c_int
        L.hssfsst_plan_check.argtypes = [vp]
        L.hssfsst_plan_check.restype = c_int
        L.hssfsst_plan_set_timing.argtypes = [vp, c_int]
        L.hssfsst_plan_set_timing.restype = c_int
        L.hssfsst_plan_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ip]
        L.hssfsst_plan_timing.restype = c_int
        L.hssfsst_dtwin.argtypes = [dp, c_int, c_dbl, dp]
        L.hssfsst_dtwin.restype = c_int
        L.hssfsst_band.argtypes = [c_int, c_dbl, c_dbl, c_dbl, ip, ip]
        L.hssfsst_band.restype = c_int
        L.hssfsst_update_mean.argtypes = [c_dbl, c_dbl, c_i64]
        L.hssfsst_update_mean.restype = c_dbl
        L.hssfsst_update_variance.argtypes = [c_dbl, c_dbl, c_dbl, c_i64]
        L.hssfsst_update_variance.restype = c_dbl
        L.hssfsst_moments_merge.argtypes = [vp, vp, c_i64, c_int, vp, vp]
        L.hssfsst_moments_merge.restype = c_int
        L.hssfsst_parse_signal_csv.argtypes = [ctypes.c_char_p, c_i64, vp, vp, c_i64]
        L.hssfsst_parse_signal_csv.restype = c_i64
        L.hssfsst_pack_recordings.argtypes = [vp, vp, c_i64, c_int, c_int, vp, c_i64, vp, c_i64, c_int]
        L.hssfsst_pack_recordings.restype = c_i64
        L.hssfsst_resample.argtypes = [dp, c_i64, c_i64, dp]
        L.hssfsst_resample.restype = c_int
        L.hssfsst_resample_plan_create.argtypes = [ctypes.POINTER(vp), c_int, c_i64, c_i64]
        L.hssfsst_resample_plan_create.restype = c_int
        L.hssfsst_resample_plan_destroy.argtypes = [vp]
        L.hssfsst_resample_plan_destroy.restype = c_int
        L.hssfsst_resample_plan_info.argtypes = [vp, vp, vp, ip, ip, ip, ip]
        L.hssfsst_resample_plan_info.restype = c_int
        L.hssfsst_resample_exec.argtypes = [vp, vp, c_int, c_i64, c_i64, vp, c_int, c_i64, c_int, vp, c_int, vp, c_int, vp]
        L.hssfsst_resample_exec.restype = c_int
        L.hssfsst_resample_plan_create_ragged.argtypes = [ctypes.POINTER(vp), c_int, c_i64]
        L.hssfsst_resample_plan_create_ragged.restype = c_int
        L.hssfsst_resample_exec_ragged.argtypes = [vp, vp, c_int, c_i64, vp, vp, c_i64, c_int, vp, c_int, vp, c_int, vp]
        L.hssfsst_resample_exec_ragged.restype = c_int
        fpp = ctypes.POINTER(ctypes.c_void_p)
        L.hssfsst_segmenter_create.argtypes = [ctypes.POINTER(vp), c_int, c_int, c_int, fpp, fpp, vp, vp]
        L.hssfsst_segmenter_create.restype = c_int
        L.hssfsst_segmenter_destroy.argtypes = [vp]
        L.hssfsst_segmenter_destroy.restype = c_int
        L.hssfsst_segmenter_info.argtypes = [vp, ip, ip, ip, ip]
        L.hssfsst_segmenter_info.restype = c_int
        L.hssfsst_segmenter_exec.argtypes = [vp, vp, c_int, c_i64, c_i64, vp, vp, vp, vp]
        L.hssfsst_segmenter_exec.restype = c_int
        L.hssfsst_segmenter_exec_ragged.argtypes = [vp, vp, c_int, ctypes.POINTER(c_i64), c_i64, vp, vp, c_int, vp, vp]
        L.hssfsst_segmenter_exec_ragged.restype = c_int
        L.hssfsst_decode_info.argtypes = [ip, ctypes.POINTER(c_i64)]
        L.hssfsst_decode_info.restype = c_int
        L.hssfsst_decode_states.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                            vp, vp, c_int, vp]
        L.hssfsst_decode_states.restype = c_int
        fp = ctypes.POINTER(ctypes.c_float)
        L.hssfsst_decode_durations_info.argtypes = [ip, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]
        L.hssfsst_decode_durations_info.restype = c_int
        L.hssfsst_decode_durations.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, fp, fp, fp, fp, c_int, vp, vp, vp, c_i64, c_int, vp]
        L.hssfsst_decode_durations.restype = c_int
        L.hssfsst_posteriors_info.argtypes = [ip, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]
        L.hssfsst_posteriors_info.restype = c_int
        L.hssfsst_posteriors.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, vp, vp, vp, vp, vp, vp, vp, vp, c_i64, c_int, vp]
        L.hssfsst_posteriors.restype = c_int
        L.hssfsst_posteriors_durations_info.argtypes = [ip, ip] + [ctypes.POINTER(c_i64)] * 4
        L.hssfsst_posteriors_durations_info.restype = c_int
        L.hssfsst_posteriors_durations.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, vp, vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp, vp, c_i64,
                                                   c_int, vp]
        L.hssfsst_posteriors_durations.restype = c_int
        L.hssfsst_posteriors_durations_counts_info.argtypes = [ctypes.POINTER(c_i64)] * 3 + [ip]
        L.hssfsst_posteriors_durations_counts_info.restype = c_int
        L.hssfsst_posteriors_durations_counts.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, vp, vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                          c_i64, c_int, vp]
        L.hssfsst_posteriors_durations_counts.restype = c_int
        L.hssfsst_score_info.argtypes = [ctypes.POINTER(c_i64)] * 3 + [ip] * 3
        L.hssfsst_score_info.restype = c_int
        L.hssfsst_score_states.argtypes = [vp, vp, vp, ctypes.POINTER(c_i64), c_i64, c_int, vp, vp, vp, vp, c_i64, ctypes.POINTER(Launch)]
        L.hssfsst_score_states.restype = c_int
        L.hssfsst_stitch_windows.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, ctypes.POINTER(c_i64), c_i64, c_int, c_int, vp, c_int, vp, vp, Launch]
        L.hssfsst_stitch_windows.restype = c_int
        L.hssfsst_bilstm_create.argtypes = [ctypes.POINTER(vp), c_int, c_int, c_int]
        L.hssfsst_bilstm_create.restype = c_int
        L.hssfsst_bilstm_destroy.argtypes = [vp]
        L.hssfsst_bilstm_destroy.restype = c_int
        L.hssfsst_bilstm_set_weights.argtypes = [vp, fpp, vp]
        L.hssfsst_bilstm_set_weights.restype = c_int
        L.hssfsst_bilstm_stash_floats.argtypes = [vp, c_i64, c_i64, ctypes.POINTER(c_i64)]
        L.hssfsst_bilstm_stash_floats.restype = c_int
        L.hssfsst_bilstm_forward.argtypes = [vp, vp, c_i64, c_i64, vp, vp, vp, vp, vp, vp, vp]
        L.hssfsst_bilstm_forward.restype = c_int
        L.hssfsst_bilstm_backward.argtypes = [vp, vp, vp, vp, vp, vp, c_i64, c_i64, vp, vp, vp, vp]
        L.hssfsst_bilstm_backward.restype = c_int
        L.hssfsst_bilstm_stash_floats_ragged.argtypes = [vp, ctypes.POINTER(c_i64), c_i64, ctypes.POINTER(c_i64)]
        L.hssfsst_bilstm_stash_floats_ragged.restype = c_int
        L.hssfsst_bilstm_forward_ragged.argtypes = [vp, vp, ctypes.POINTER(c_i64), c_i64, vp, vp, vp, vp, vp, vp, vp]
        L.hssfsst_bilstm_forward_ragged.restype = c_int
        L.hssfsst_bilstm_backward_ragged.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(c_i64), c_i64, vp, vp, vp, vp]
        L.hssfsst_bilstm_backward_ragged.restype = c_int
        L.hssfsst_device_count.restype = c_int
        L.hssfsst_version.restype = c_int
        L.hssfsst_last_error.restype = ctypes.c_char_p
        _lib = L
        return _lib


def check(rc: int, what: str) -> None:
    """Status -> exception: bad arguments raise ValueError, everything else -- including a
    configuration the kernels cannot run (E_UNSUPPORTED) -- RuntimeError, the one exception the
    reference's dataset catches around the transform (hss/datasets/heart_sounds.py:183)."""
    if rc == 0:
        return
    msg = lib().hssfsst_last_error().decode("utf-8", "replace")
    if rc == E_INVAL:
        raise ValueError(f"{what}: {msg} (status {rc})")
    raise RuntimeError(f"{what}: {msg} (status {rc})")


WHOLE_RECORDINGS = (0x7fffffff, 1)     # the (stride, n) pair under which every recording is one "frame": its start, nothing else


def pack_recordings(ptrs, lens, stage, starts, expected: int, stride: int = WHOLE_RECORDINGS[0], n: int = WHOLE_RECORDINGS[1]) -> None:
    """``hssfsst_pack_recordings``: the host float32 recordings behind ``ptrs`` (uint64 array; ``lens`` int64 array) are copied back
    to back into the tensor ``stage`` (threaded), and the starts of their ``n``-sample frames at ``stride`` -- by default of the
    recordings themselves -- are written to the int64 array ``starts``.  ``expected``: the number of starts the caller counted;
    any other return is the library's error, or a ValueError."""
    count = int(lens.shape[0])
    got = lib().hssfsst_pack_recordings(ctypes.c_void_p(ptrs.ctypes.data), ctypes.c_void_p(lens.ctypes.data), count, int(stride), int(n),
                                        ctypes.c_void_p(stage.data_ptr()), int(stage.numel()),
                                        ctypes.c_void_p(starts.ctypes.data), int(starts.shape[0]), 0)
    if got != expected:
        check(int(got) if got < 0 else E_INVAL, "hssfsst_pack_recordings")
