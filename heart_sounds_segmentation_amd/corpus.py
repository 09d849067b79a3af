"""Batched counterpart of the reference's in-memory dataset loop:
``DavidSpringerHSS.__init__`` (/root/reference/hss/datasets/heart_sounds.py:155-169) turns every
recording into frames (``frame_signal``, stride 1000, length 2000) and calls the transform once per
frame on the CPU.  Here recordings are uploaded ONCE, in groups laid back to back in one buffer, and all frames of a
group are transformed by one call (``hssfsst_exec_list``: no 2x duplicated H2D copy of the overlapping frames; a single
recording's frames can also be read in place with ``hssfsst_exec_frames`` via ``FSST.batch(frame_batch(x))``).

Semantics kept (pinned by tests/golden/frame_signal.npz): recordings shorter than ``frame_len`` are
skipped (heart_sounds.py:161-162); ``L = floor((T - n)/stride)`` frames -- one fewer than fit --
(preprocess.py:40,48-52); labels are shifted to 0-based (``y - 1``, heart_sounds.py:164) and framed
identically; each item is ``(features (n, 2K) float32, labels (n,) int64)`` (heart_sounds.py:168).

How it is fed (round 3; round 2 moved 77.7 k windows/s from host recordings against 3.98 M/s device-resident):
  * ONE feature arena ``(frames, n, 2K)`` per call -- on the device, or in (pinned) host memory when the caller wants
    host tensors -- and ONE label arena; the returned ``FrameItems`` hands out views of them on demand (the reference's
    list of 26 136 tuples is built only if somebody asks for ``list(items)``);
  * the recordings of a group are packed into one of two PINNED staging buffers and uploaded on a side stream while
    the previous group is transformed (``hssfsst_exec_list`` writes straight into the group's rows of the arena);
  * host-returned features leave the device group by group on a third stream, overlapping the next group's transform.

With ``resample=Resample(num)`` the builder is the reference's ``Compose([Resample(num), FSST(...)])`` under ``framing=True``
(heart_sounds.py:166-168,199-212): every ``frame_len``-sample frame is resampled to ``num`` samples on the device (list form of
``hssfsst_resample_exec`` over the packed group), the ``(frames, num)`` buffer goes through the transform, and items are
``(num, 2K)`` features with ``(num,)`` labels ``round(Resample(frame of (y - 1))) - 1`` -- the reference's double shift kept --
computed on the device from a second packed upload of the label tracks.

Whole recordings (``build_recordings``): the reference's OTHER way to feed the model, ``DavidSpringerHSS(in_memory=False)``
(heart_sounds.py:175-184,199-212) and ``PhysionetChallenge2016`` (:85-106), transform each whole recording in its own call.  Here a
corpus of them is transformed in groups of at most ``max_samples`` samples, one ``hssfsst_exec_ragged`` call per group (signals of
different lengths: one transform launch plus the z-score), uploads double-buffered as above.  Items are the lazy dataset's
``(features (T, 2K) or (T, K), y unchanged or None)``: every recording, the short ones included, and no label shift.

Whole recordings resampled (``build_resampled_recordings``): the lazy dataset with ``Compose([Resample(num), FSST(...)])`` (heart_sounds.py:
175-184,199-212), where every item is ``(FSST(Resample(num)(x)), round(Resample(num)(y)) - 1)`` of ``num`` samples.  Groups of at most
``max_samples`` input samples are packed and uploaded as above (label tracks in a second staging pair); each group is ONE ragged
resample call (``hssfsst_resample_exec_ragged``: recordings of different lengths, every one to ``num``) into a ``(count, num)``
buffer, one ``FSST.batch`` call on it, and one ragged call with the label rule on the tracks.  Items are views of one
``(count, num, C)`` arena (``FrameItems``).  ``build_recordings(resample=)`` keeps refusing: its items keep their own lengths.

Multi-GPU (BASELINE config C3): ``rank`` / ``world`` split the RECORDINGS in contiguous
blocks (``dist.shard_bounds``), so framing stays local to a rank and concatenating the ranks' item lists in rank
order is the single-process list; ``gather_features`` reassembles the feature tensor on every rank with one
(ragged) RCCL all-gather on the process group's device; a rank without frames takes part with an empty block.
"""
from __future__ import annotations

from collections.abc import Sequence as _SequenceABC
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dist as hdist
from .framing import frame_batch, frame_starts

Item = Tuple[torch.Tensor, Optional[torch.Tensor]]


class FrameItems(_SequenceABC):
    """The reference dataset's ``self.data`` -- a sequence of ``(features (n, 2K), labels (n,) or None)`` -- as views of
    one feature arena and one label arena (no per-item allocation; ``items[i]``, ``len``, iteration and slicing work as
    on the reference's list)."""

    def __init__(self, features: torch.Tensor, labels: Optional[torch.Tensor]):
        self.features = features                          # (frames, n, 2K) float32 (or the transform's out_dtype), device or host
        self.labels = labels                              # (frames, n) int64 on the host, or None

    def __len__(self) -> int:
        return int(self.features.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self.features[i], (self.labels[i] if self.labels is not None else None)


class CorpusBuilder:
    """The builder as an object: keeps its pinned staging buffers, device staging, streams and (when asked) the feature
    arena between calls, so that a second corpus of the same size pays for no allocation (page-locking the host
    buffers and hipMalloc of gigabytes cost more than the transform itself)."""

    def __init__(self, fsst, stride: int = 1000, frame_len: int = 2000, device: Optional[torch.device] = None,
                 windows_per_launch: int = 4096, pin_host: bool = True, resample=None):
        self.fsst, self.stride, self.frame_len = fsst, int(stride), int(frame_len)
        self.resample = resample                          # a Resample: frames are resampled to resample.num samples first
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.wpl, self.pin_host = int(windows_per_launch), bool(pin_host)
        self._cap_samples = self._cap_frames = self._cap_ring = 0
        self._cap_rs = self._cap_lab = 0
        self._bufs = None

    def _ensure_resample(self, max_samples: int, max_frames: int, num: int, need_labels: bool) -> None:
        """Device buffer of a group's resampled frames; pinned / device staging of its label tracks."""
        b, dev = self._bufs, self.dev
        if max_frames * num > self._cap_rs:
            b["rs_d"] = torch.empty(max_frames * num, dtype=torch.float32, device=dev)
            self._cap_rs = max_frames * num
        if need_labels and max_samples > self._cap_lab:
            b["lab_h"] = [torch.empty(max_samples, dtype=torch.float32, pin_memory=True) for _ in range(2)]
            b["lab_d"] = [torch.empty(max_samples, dtype=torch.float32, device=dev) for _ in range(2)]
            b["lab_starts"] = np.empty(max_frames, dtype=np.int64)
            self._cap_lab = max_samples
        elif need_labels and b["lab_starts"].shape[0] < max_frames:
            b["lab_starts"] = np.empty(max_frames, dtype=np.int64)

    def _ensure(self, max_samples: int, max_frames: int, C: int, need_ring: bool, item_len: Optional[int] = None,
                dtype: torch.dtype = torch.float32) -> None:
        dev = self.dev
        if self._bufs is None:
            self._bufs = {"up": torch.cuda.Stream(dev), "down": torch.cuda.Stream(dev),
                          "up_done": [torch.cuda.Event() for _ in range(2)], "used": [torch.cuda.Event() for _ in range(2)],
                          "ring_free": [torch.cuda.Event() for _ in range(2)]}
        b = self._bufs
        if max_samples > self._cap_samples:
            b["stage_h"] = [torch.empty(max_samples, dtype=torch.float32, pin_memory=True) for _ in range(2)]
            b["stage_d"] = [torch.empty(max_samples, dtype=torch.float32, device=dev) for _ in range(2)]
            self._cap_samples = max_samples
        if max_frames > self._cap_frames:
            b["start_h"] = [torch.empty(max_frames, dtype=torch.int64, pin_memory=True) for _ in range(2)]
            b["start_d"] = [torch.empty(max_frames, dtype=torch.int64, device=dev) for _ in range(2)]
            self._cap_frames = max_frames
        item_len = self.frame_len if item_len is None else item_len
        if need_ring and (max_frames * C > self._cap_ring or b["ring_d"][0].shape[1] != item_len or b["ring_d"][0].dtype != dtype):
            b["ring_d"] = [torch.empty((max_frames, item_len, C), dtype=dtype, device=dev) for _ in range(2)]
            self._cap_ring = max_frames * C

    def build_recordings(self, recordings: Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]], keep_on_device: bool = False,
                         max_samples: int = 1 << 25) -> "RecordingItems":
        """See the module function ``build_recordings``."""
        fsst, dev = self.fsst, self.dev
        if self.resample is not None:
            raise ValueError("CorpusBuilder.build_recordings: resample= is not supported for whole recordings (every recording length "
                             "needs a resample plan of its own); resample the recordings first")
        if not (getattr(fsst, "stack", False) or getattr(fsst, "abs", False)):
            raise ValueError("CorpusBuilder.build_recordings: the transform must have stack=True or abs=True (time-major float32 "
                             "features); for the raw complex transform call FSST.ragged")
        if dev.type != "cuda":
            raise ValueError("CorpusBuilder.build_recordings: the builder's device is not a HIP device")
        recs: Sequence = recordings if isinstance(recordings, (list, tuple)) else list(recordings)
        xs = []
        for i, (x, _) in enumerate(recs):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
            if t.ndim == 2 and t.shape[-1] == 1:
                t = t[:, 0]
            if t.ndim != 1 or t.shape[0] < 1:
                raise ValueError(f"CorpusBuilder.build_recordings: recording {i} has shape {tuple(x.shape)}; expected (T,) or (T, 1), T >= 1")
            xs.append(t)
        ys = [y if (y is None or isinstance(y, torch.Tensor)) else torch.as_tensor(np.asarray(y)) for _, y in recs]
        lens_np = np.asarray([int(t.shape[0]) for t in xs], dtype=np.int64)
        total = int(lens_np.sum())
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens_np)]).astype(np.int64))
        from .transforms.synchrosqueeze import RaggedFeatures
        plan = fsst._plan(fsst._device_index(torch.empty(0, device=dev)))
        C, K, fdt = plan.ofps, plan.K, plan.out_dtype     # (fdt: the features' element type -- a half STACK transform's out_dtype)
        if keep_on_device:
            feats = torch.empty((total, C), dtype=fdt, device=dev)
        else:
            try:
                feats = torch.empty((total, C), dtype=fdt, pin_memory=bool(self.pin_host and total > 0))
            except RuntimeError:                          # page-locking that much memory can be refused: pageable then
                feats = torch.empty((total, C), dtype=fdt)
        items = RecordingItems(RaggedFeatures(feats, offsets, K, False), ys)
        if total == 0:
            return items
        # groups of at most max_samples samples (a longer recording is a group of its own)
        groups: List[Tuple[int, int]] = []
        g0, acc = 0, 0
        for i, T in enumerate(lens_np.tolist()):
            if acc > 0 and acc + T > max_samples:
                groups.append((g0, i))
                g0, acc = i, 0
            acc += T
        groups.append((g0, len(xs)))
        pos_np = np.concatenate([[0], np.cumsum(lens_np)])
        max_group = max(int(pos_np[b] - pos_np[a]) for a, b in groups)
        self._ensure(max_group, 0, C, False)
        B = self._bufs
        if not keep_on_device and (B.get("rec_ring") is None or B["rec_ring"][0].numel() < max_group * C or B["rec_ring"][0].dtype != fdt):
            B["rec_ring"] = [torch.empty(max_group * C, dtype=fdt, device=dev) for _ in range(2)]
        main, up, down = torch.cuda.current_stream(dev), B["up"], B["down"]
        stage_h, stage_d = B["stage_h"], B["stage_d"]
        up_done, used, ring_free = B["up_done"], B["used"], B["ring_free"]
        up.wait_stream(main)
        from . import _lib
        import ctypes
        held = [t if (t.dtype == torch.float32 and t.is_contiguous() and not t.is_cuda) else t.detach().to("cpu", torch.float32).contiguous()
                for t in xs]                               # (device recordings are staged through the host like the rest: rare)
        ptrs_np = np.asarray([t.data_ptr() for t in held], dtype=np.uint64)
        L = _lib.lib()
        starts_np = np.empty(len(xs), dtype=np.int64)

        def pack(gi: int) -> int:
            """Host side of group gi: recordings back to back into pinned staging (one threaded native call); upload on `up`."""
            a, b = groups[gi]
            buf = gi & 1
            if gi >= 2:
                used[buf].synchronize()                  # the transform of group gi - 2 no longer reads this staging buffer
            n = int(pos_np[b] - pos_np[a])
            got = L.hssfsst_pack_recordings(ctypes.c_void_p(ptrs_np[a:b].ctypes.data), ctypes.c_void_p(lens_np[a:b].ctypes.data), b - a,
                                            0x7fffffff, 1, ctypes.c_void_p(stage_h[buf].data_ptr()), int(stage_h[buf].numel()),
                                            ctypes.c_void_p(starts_np[a:b].ctypes.data), b - a, 0)
            if got != b - a:
                _lib.check(int(got) if got < 0 else _lib.E_INVAL, "hssfsst_pack_recordings")
            with torch.cuda.stream(up):
                stage_d[buf][:n].copy_(stage_h[buf][:n], non_blocking=True)
                up_done[buf].record(up)
            return n

        n = pack(0)
        for gi, (a, b) in enumerate(groups):
            buf = gi & 1
            r0, r1 = int(pos_np[a]), int(pos_np[b])
            main.wait_event(up_done[buf])
            if keep_on_device:
                dst = feats[r0:r1]
            else:
                if gi >= 2:
                    main.wait_event(ring_free[buf])
                dst = B["rec_ring"][buf][:n * C].view(n, C)
            fsst.ragged(stage_d[buf][:n], lengths=lens_np[a:b], out=dst)
            used[buf].record(main)
            if not keep_on_device:
                down.wait_stream(main)
                with torch.cuda.stream(down):
                    feats[r0:r1].copy_(dst, non_blocking=True)
                    ring_free[buf].record(down)
            if gi + 1 < len(groups):
                n = pack(gi + 1)                         # host packing + upload of the next group overlap this transform
        if not keep_on_device:
            down.synchronize()
        main.synchronize()
        fsst.check()
        return items

    def build_resampled_recordings(self, recordings: Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]], keep_on_device: bool = False,
                                   max_samples: int = 1 << 25) -> FrameItems:
        """See the module function ``build_resampled_recordings`` (the builder's ``resample`` is the ``Resample``)."""
        fsst, dev, rsm = self.fsst, self.dev, self.resample
        name = "CorpusBuilder.build_resampled_recordings"
        # ---- arguments, all checked before a plan (or the GPU) is touched
        if rsm is None:
            raise ValueError(f"{name}: the builder has no resample= (a Resample(num))")
        if not (getattr(fsst, "stack", False) or getattr(fsst, "abs", False)):
            raise ValueError(f"{name}: the transform must have stack=True or abs=True (time-major float32 features)")
        if dev.type != "cuda":
            raise ValueError(f"{name}: the builder's device is not a HIP device")
        num = int(rsm.num)
        if num < 1:
            raise ValueError(f"{name}: Resample.num must be >= 1, got {num}")
        recs: Sequence = recordings if isinstance(recordings, (list, tuple)) else list(recordings)
        xs, ys = [], []
        for i, (x, y) in enumerate(recs):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
            if t.ndim == 2 and t.shape[-1] == 1:
                t = t[:, 0]
            if t.ndim != 1 or t.shape[0] < 1 or t.is_complex():
                raise ValueError(f"{name}: recording {i} has shape {tuple(t.shape)} ({t.dtype}); expected real (T,) or (T, 1), T >= 1")
            if y is not None:
                y = (y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))).reshape(-1)
                if y.shape[0] != t.shape[0] or y.is_complex():
                    raise ValueError(f"{name}: the labels of recording {i} are {tuple(y.shape)} ({y.dtype}), the recording {tuple(t.shape)}")
            xs.append(t)
            ys.append(y)
        has = [y is not None for y in ys]
        if 0 < sum(has) < len(has):
            raise ValueError(f"{name}: some recordings carry labels and some do not; pass labels for all or for none")
        have_labels = len(has) > 0 and all(has)
        lens_np = np.asarray([int(t.shape[0]) for t in xs], dtype=np.int64)
        count = len(xs)
        plan = fsst._plan(fsst._device_index(torch.empty(0, device=dev)))
        C, fdt = plan.ofps, plan.out_dtype               # (fdt: the features' element type -- a half STACK transform's out_dtype)
        shape = (count, num, C)
        if keep_on_device:
            feats = torch.empty(shape, dtype=fdt, device=dev)
        else:
            try:
                feats = torch.empty(shape, dtype=fdt, pin_memory=bool(self.pin_host and count > 0))
            except RuntimeError:                          # page-locking that much memory can be refused: pageable then
                feats = torch.empty(shape, dtype=fdt)
        if count == 0:
            return FrameItems(feats, None)
        # groups of at most max_samples input samples (a longer recording is a group of its own)
        groups: List[Tuple[int, int]] = []
        g0, acc = 0, 0
        for i, T in enumerate(lens_np.tolist()):
            if acc > 0 and acc + T > max_samples:
                groups.append((g0, i))
                g0, acc = i, 0
            acc += T
        groups.append((g0, count))
        pos_np = np.concatenate([[0], np.cumsum(lens_np)])
        max_group = max(int(pos_np[b] - pos_np[a]) for a, b in groups)
        max_cnt = max(b - a for a, b in groups)
        self._ensure(max_group, max_cnt, C, not keep_on_device, num, fdt)
        self._ensure_resample(max_group, max_cnt, num, have_labels)
        B = self._bufs
        lab_d = torch.empty((count, num), dtype=torch.int64, device=dev) if have_labels else None
        main, up, down = torch.cuda.current_stream(dev), B["up"], B["down"]
        stage_h, stage_d = B["stage_h"], B["stage_d"]
        up_done, used, ring_free = B["up_done"], B["used"], B["ring_free"]
        up.wait_stream(main)                             # (the staging buffers may still be read by an earlier call's work)
        from . import _lib
        import ctypes
        held = [t if (t.dtype == torch.float32 and t.is_contiguous() and not t.is_cuda) else t.detach().to("cpu", torch.float32).contiguous()
                for t in xs]                               # (device recordings are staged through the host like the rest: rare)
        ptrs_np = np.asarray([t.data_ptr() for t in held], dtype=np.uint64)
        if have_labels:                                  # the label tracks as given (no shift), exact in float32, packed like the signals
            held_y = [y.to("cpu", torch.float32).contiguous() for y in ys]
            yptrs_np = np.asarray([y.data_ptr() for y in held_y], dtype=np.uint64)
        L = _lib.lib()
        starts_np = np.empty(count, dtype=np.int64)

        def pack(gi: int) -> int:
            """Host side of group gi: recordings (and label tracks) back to back into pinned staging; upload on `up`."""
            a, b = groups[gi]
            buf = gi & 1
            if gi >= 2:
                used[buf].synchronize()                  # the calls of group gi - 2 no longer read this staging pair
            n = int(pos_np[b] - pos_np[a])
            for ptrs, dst in ((ptrs_np, stage_h[buf]),) + (((yptrs_np, B["lab_h"][buf]),) if have_labels else ()):
                got = L.hssfsst_pack_recordings(ctypes.c_void_p(ptrs[a:b].ctypes.data), ctypes.c_void_p(lens_np[a:b].ctypes.data), b - a,
                                                0x7fffffff, 1, ctypes.c_void_p(dst.data_ptr()), int(dst.numel()),
                                                ctypes.c_void_p(starts_np[a:b].ctypes.data), b - a, 0)
                if got != b - a:
                    _lib.check(int(got) if got < 0 else _lib.E_INVAL, "hssfsst_pack_recordings")
            with torch.cuda.stream(up):
                stage_d[buf][:n].copy_(stage_h[buf][:n], non_blocking=True)
                if have_labels:
                    B["lab_d"][buf][:n].copy_(B["lab_h"][buf][:n], non_blocking=True)
                up_done[buf].record(up)
            return n

        n = pack(0)
        for gi, (a, b) in enumerate(groups):
            buf = gi & 1
            main.wait_event(up_done[buf])
            if keep_on_device:
                dst = feats[a:b]
            else:
                if gi >= 2:
                    main.wait_event(ring_free[buf])
                dst = B["ring_d"][buf][:b - a]
            rs = B["rs_d"][:(b - a) * num].view(b - a, num)
            rsm.ragged(stage_d[buf][:n], lengths=lens_np[a:b], out=rs)
            fsst.batch(rs, out=dst)
            if have_labels:
                rsm.ragged(B["lab_d"][buf][:n], lengths=lens_np[a:b], labels=True, out=lab_d[a:b])
            used[buf].record(main)
            if not keep_on_device:
                down.wait_stream(main)
                with torch.cuda.stream(down):
                    feats[a:b].copy_(dst, non_blocking=True)
                    ring_free[buf].record(down)
            if gi + 1 < len(groups):
                n = pack(gi + 1)                         # host packing + upload of the next group overlap these calls
        if not keep_on_device:
            down.synchronize()
        main.synchronize()
        fsst.check()
        return FrameItems(feats, lab_d.cpu() if have_labels else None)

    def build(self, recordings: Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]], keep_on_device: bool = False,
              rank: Optional[int] = None, world: Optional[int] = None, out: Optional[torch.Tensor] = None) -> FrameItems:
        """See ``build_features``.  ``out``: a feature arena of a previous call to write into (same shape, device arena
        for ``keep_on_device`` else host)."""
        fsst, stride, frame_len, dev = self.fsst, self.stride, self.frame_len, self.dev
        rsm = self.resample
        if rsm is not None and dev.type != "cuda":
            raise ValueError("CorpusBuilder.build: resample= runs on a HIP device; the builder's device is not one")
        out_len = int(rsm.num) if rsm is not None else frame_len     # samples per item after the optional resampling
        recs: Sequence = recordings if isinstance(recordings, (list, tuple)) else list(recordings)
        # argument errors are properties of the WHOLE call and are raised before the list is cut to this rank's shard: a rank that
        # raised alone left the others waiting in the gather that follows
        if dev.type == "cuda" and not (getattr(fsst, "stack", False) or getattr(fsst, "abs", False)):
            # (the raw transform is complex64 (frames, K, n), frequency-major: not the time-major float32 arena this builder fills)
            raise ValueError("CorpusBuilder.build: the transform must have stack=True or abs=True (time-major float32 features); "
                             "for the raw complex transform call FSST.frames per group of recordings")
        kept_all = [y is not None for x, y in recs if x.shape[0] >= frame_len]
        if 0 < sum(kept_all) < len(kept_all):
            raise ValueError("CorpusBuilder.build: some recordings carry labels and some do not; pass labels for all or for none")
        if world is not None and world > 1:
            lo, hi = hdist.shard_bounds(len(recs), int(world), int(rank or 0))
            recs = recs[lo:hi]
        recs = [(x.reshape(-1), y) for x, y in recs if x.shape[0] >= frame_len]       # heart_sounds.py:161-162
        lens_np = np.asarray([int(x.shape[0]) for x, _ in recs], dtype=np.int64)
        L_np = (lens_np - frame_len) // stride                                           # frame_signal: one fewer than fit
        nfr_np = np.where(L_np <= 0, 1, L_np).astype(np.int64)
        nfr = [int(v) for v in nfr_np]
        total = int(nfr_np.sum())
        # (decided on the WHOLE list, before the cut: the same answer on every rank -- a rank whose shard holds no frames returns an
        #  empty (0, frame_len) int64 tensor, not None, when the corpus is labelled, so that a gather of the labels finds every rank in it)
        have_labels = len(kept_all) > 0 and all(kept_all)
        # groups of about `windows_per_launch` frames (a launch per recording -- 33 frames -- leaves the chip idle)
        groups: List[Tuple[int, int]] = []
        g0, acc = 0, 0
        for i, k in enumerate(nfr):
            acc += k
            if acc >= self.wpl:
                groups.append((g0, i + 1))
                g0, acc = i + 1, 0
        if g0 < len(recs):
            groups.append((g0, len(recs)))
        labels = torch.empty((total, out_len), dtype=torch.int64) if have_labels and rsm is None else None

        def fill_labels(a: int, b: int, row: int) -> None:
            for i in range(a, b):
                labels[row:row + nfr[i]] = frame_batch(recs[i][1] - 1, stride, frame_len)
                row += nfr[i]

        if dev.type != "cuda":
            # host-only stand-in transforms (tests of the grouping / framing logic): one synchronous call per group
            feats = None
            row = 0
            for a, b in groups:
                xs = [recs[i][0].to(torch.float32) for i in range(a, b)]
                st, base = [], 0
                for i, x in zip(range(a, b), xs):
                    st.append(torch.from_numpy(frame_starts(int(x.shape[0]), stride, frame_len)[0]) + base)
                    base += int(x.shape[0])
                blk = fsst.frames(torch.cat(xs), torch.cat(st), frame_len)
                if feats is None:
                    feats = torch.empty((total,) + tuple(blk.shape[1:]), dtype=blk.dtype)
                feats[row:row + blk.shape[0]] = blk
                if labels is not None:
                    fill_labels(a, b, row)
                row += int(blk.shape[0])
            if feats is None:
                feats = torch.empty((0, frame_len, 0), dtype=torch.float32)
            return FrameItems(feats, labels)

        plan = fsst._plan(fsst._device_index(torch.empty(0, device=dev)))
        C, fdt = plan.ofps, plan.out_dtype              # (fdt: the features' element type -- a half STACK transform's out_dtype)
        shape = (total, out_len, C)
        if out is not None and (tuple(out.shape) != shape or out.dtype != fdt or not out.is_contiguous()
                                or out.is_cuda != bool(keep_on_device)):
            raise ValueError(f"CorpusBuilder.build: out must be a contiguous {fdt} {shape} arena "
                             f"{'on the device' if keep_on_device else 'in host memory'}")
        feats = out
        if feats is None:
            if keep_on_device:
                feats = torch.empty(shape, dtype=fdt, device=dev)
            else:
                try:
                    feats = torch.empty(shape, dtype=fdt, pin_memory=bool(self.pin_host and total > 0))
                except RuntimeError:                      # page-locking that much memory can be refused: pageable then
                    feats = torch.empty(shape, dtype=fdt)
        if total == 0:
            if have_labels and rsm is not None:
                labels = torch.empty((0, out_len), dtype=torch.int64)
            return FrameItems(feats, labels)
        max_samples = max(sum(int(recs[i][0].shape[0]) for i in range(a, b)) for a, b in groups)
        max_frames = max(sum(nfr[a:b]) for a, b in groups)
        self._ensure(max_samples, max_frames, C, not keep_on_device, out_len, fdt)
        dev_labels = have_labels and rsm is not None     # labels resampled on the device: (total, num) device arena, copied once
        if rsm is not None:
            self._ensure_resample(max_samples, max_frames, out_len, dev_labels)
        B = self._bufs
        lab_d = torch.empty((total, out_len), dtype=torch.int64, device=dev) if dev_labels else None
        main, up, down = torch.cuda.current_stream(dev), B["up"], B["down"]
        stage_h, stage_d, start_h, start_d = B["stage_h"], B["stage_d"], B["start_h"], B["start_d"]
        up_done, used, ring_free = B["up_done"], B["used"], B["ring_free"]
        ring_d = B.get("ring_d")
        up.wait_stream(main)                             # (the staging buffers may still be read by an earlier call's work)

        # the host side of a group is ONE native call (hssfsst_pack_recordings: threaded copies into the pinned staging
        # buffer + the frame starts): per recording Python does nothing but hand over a pointer.  (Per-recording copy_ /
        # numpy calls were 0.29 ms per recording: 115 k windows/s however fast the device is.)
        from . import _lib
        import ctypes
        held = [x if (x.dtype == torch.float32 and x.is_contiguous() and not x.is_cuda) else x.detach().to("cpu", torch.float32).contiguous()
                for x, _ in recs]
        ptrs_np = np.asarray([x.data_ptr() for x in held], dtype=np.uint64)
        if dev_labels:                                   # the label tracks (y - 1), exact in float32, packed like the signals
            held_y = [(y.reshape(-1) - 1).to("cpu", torch.float32).contiguous() for _, y in recs]
            yptrs_np = np.asarray([y.data_ptr() for y in held_y], dtype=np.uint64)
        pos_np = np.concatenate([[0], np.cumsum(lens_np)])
        fr_np = np.concatenate([[0], np.cumsum(nfr_np)])
        L = _lib.lib()

        def pack(gi: int) -> Tuple[int, int]:
            """Host side of group gi: recordings back to back into pinned staging, frame starts; upload on `up`."""
            a, b = groups[gi]
            buf = gi & 1
            if gi >= 2:
                used[buf].synchronize()                  # the transform of group gi - 2 no longer reads this staging pair
            pos, nf = int(pos_np[b] - pos_np[a]), int(fr_np[b] - fr_np[a])
            got = L.hssfsst_pack_recordings(ctypes.c_void_p(ptrs_np[a:b].ctypes.data), ctypes.c_void_p(lens_np[a:b].ctypes.data), b - a,
                                            stride, frame_len, ctypes.c_void_p(stage_h[buf].data_ptr()), int(stage_h[buf].numel()),
                                            ctypes.c_void_p(start_h[buf].data_ptr()), int(start_h[buf].numel()), 0)
            if got != nf:
                _lib.check(int(got) if got < 0 else _lib.E_INVAL, "hssfsst_pack_recordings")
            if dev_labels:
                lab_h, lst = B["lab_h"][buf], B["lab_starts"]
                got = L.hssfsst_pack_recordings(ctypes.c_void_p(yptrs_np[a:b].ctypes.data), ctypes.c_void_p(lens_np[a:b].ctypes.data), b - a,
                                                stride, frame_len, ctypes.c_void_p(lab_h.data_ptr()), int(lab_h.numel()),
                                                ctypes.c_void_p(lst.ctypes.data), int(lst.shape[0]), 0)
                if got != nf:
                    _lib.check(int(got) if got < 0 else _lib.E_INVAL, "hssfsst_pack_recordings")
            with torch.cuda.stream(up):
                stage_d[buf][:pos].copy_(stage_h[buf][:pos], non_blocking=True)
                start_d[buf][:nf].copy_(start_h[buf][:nf], non_blocking=True)
                if dev_labels:
                    B["lab_d"][buf][:pos].copy_(B["lab_h"][buf][:pos], non_blocking=True)
                up_done[buf].record(up)
            return pos, nf

        row = 0
        sizes = pack(0)
        for gi in range(len(groups)):
            buf = gi & 1
            pos, nf = sizes
            main.wait_event(up_done[buf])
            if keep_on_device:
                dst = feats[row:row + nf]
            else:
                if gi >= 2:
                    main.wait_event(ring_free[buf])
                dst = ring_d[buf][:nf]
            if rsm is None:
                fsst.frames(stage_d[buf][:pos], start_d[buf][:nf], frame_len, out=dst)
            else:
                rs = B["rs_d"][:nf * out_len].view(nf, out_len)
                rsm.frames(stage_d[buf][:pos], start_d[buf][:nf], frame_len, out=rs)
                fsst.batch(rs, out=dst)
                if dev_labels:
                    rsm.frames(B["lab_d"][buf][:pos], start_d[buf][:nf], frame_len, labels=True, out=lab_d[row:row + nf])
            used[buf].record(main)
            if not keep_on_device:
                down.wait_stream(main)
                with torch.cuda.stream(down):
                    feats[row:row + nf].copy_(dst, non_blocking=True)
                    ring_free[buf].record(down)
            if gi + 1 < len(groups):
                sizes = pack(gi + 1)                     # host packing + upload of the next group overlap this transform
            if labels is not None and not dev_labels:    # (host work, also overlapped)
                fill_labels(groups[gi][0], groups[gi][1], row)
            row += nf
        if not keep_on_device:
            down.synchronize()
        main.synchronize()
        fsst.check()
        if dev_labels:
            labels = lab_d.cpu()
        return FrameItems(feats, labels)


def build_features(recordings: Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]], fsst,
                   stride: int = 1000, frame_len: int = 2000, device: Optional[torch.device] = None,
                   keep_on_device: bool = False, rank: Optional[int] = None,
                   world: Optional[int] = None, windows_per_launch: int = 4096, pin_host: bool = True,
                   resample=None) -> FrameItems:
    """``recordings``: iterable of ``(x (T,) float32, y (T,) int64 labels in 1..4 or None)``.
    Returns what the reference dataset would hold in ``self.data`` (``in_memory=True, framing=True``);
    with ``world`` > 1 only the part of it that comes from this rank's block of recordings.
    ``keep_on_device=True`` leaves the features on the GPU (a GPU consumer follows: BASELINE config C4);
    otherwise they are returned in host memory (pinned when ``pin_host``), as the reference's CPU tensors.
    ``resample=Resample(num)``: every frame is resampled to ``num`` samples before the transform (see the module notes).
    (One-shot form of ``CorpusBuilder``, which keeps its staging buffers between calls.)"""
    return CorpusBuilder(fsst, stride, frame_len, device, windows_per_launch, pin_host, resample).build(
        recordings, keep_on_device=keep_on_device, rank=rank, world=world)


class RecordingItems(_SequenceABC):
    """The lazy dataset's items for a whole corpus -- ``[ds[i] for i in range(len(ds))]`` of
    ``DavidSpringerHSS(in_memory=False, transform=Compose([FSST(...)]))`` (heart_sounds.py:175-184) -- as views of one feature arena:
    item i is ``(features (T_i, C), labels_i)`` with the recording's labels as given (or None)."""

    def __init__(self, features, labels: List[Optional[torch.Tensor]]):
        self.features = features                          # RaggedFeatures: arena (sum T_i, C), offsets
        self.labels = labels

    def __len__(self) -> int:
        return len(self.labels)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self.features[i], self.labels[i]


def build_recordings(recordings: Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]], fsst, device: Optional[torch.device] = None,
                     keep_on_device: bool = False, pin_host: bool = True, max_samples: int = 1 << 25, resample=None) -> RecordingItems:
    """``recordings``: iterable of ``(x (T,) float32, y (T,) labels or None)``, any lengths.  Returns what the reference's lazy
    dataset (``in_memory=False``) hands out item by item: ``(fsst(x), y)`` for EVERY recording (no ``frame_len`` skip, labels
    unchanged -- no ``- 1``), as views of one arena on the device (``keep_on_device``) or in (pinned) host memory.  ``fsst`` must
    have ``stack=True`` or ``abs=True``.  Groups of at most ``max_samples`` samples go through one ``FSST.ragged`` call each.
    ``resample=`` is refused here: with a ``Resample`` every item has ``num`` samples -- call ``build_resampled_recordings``."""
    if resample is not None:
        raise ValueError("build_recordings: resample= is not supported for whole recordings (every recording length needs a "
                         "resample plan of its own); resample the recordings first")
    return CorpusBuilder(fsst, device=device, pin_host=pin_host).build_recordings(recordings, keep_on_device=keep_on_device,
                                                                                 max_samples=max_samples)


def build_resampled_recordings(recordings: Iterable[Tuple[torch.Tensor, Optional[torch.Tensor]]], fsst, resample,
                               device: Optional[torch.device] = None, keep_on_device: bool = False, pin_host: bool = True,
                               max_samples: int = 1 << 25) -> FrameItems:
    """``recordings``: iterable of ``(x (T,) float32, y (T,) labels or None)``, any lengths; ``resample``: a ``Resample(num)``.
    Returns what the reference's lazy dataset with ``Compose([resample, fsst])`` hands out item by item (``in_memory=False``,
    heart_sounds.py:175-184,199-212): ``(features (num, C), labels (num,) int64)`` for EVERY recording, the labels
    ``round(resample(y)) - 1`` of the track as given (no other shift), or None -- as a ``FrameItems`` over one ``(count, num, C)``
    arena on the device (``keep_on_device``) or in (pinned) host memory, and a ``(count, num)`` host label arena.  Labels for all
    recordings or for none.  Groups of at most ``max_samples`` input samples go through one ``Resample.ragged`` call and one
    ``FSST.batch`` call each: the features are bit-identical to ``fsst.batch(resample.ragged(xs))``."""
    return CorpusBuilder(fsst, device=device, pin_host=pin_host, resample=resample).build_resampled_recordings(
        recordings, keep_on_device=keep_on_device, max_samples=max_samples)


def gather_features(items, group=None, out_device: Optional[torch.device] = None) -> torch.Tensor:
    """All-gather this rank's features (rank order == recording order) into the full ``(windows, n, 2K)`` tensor on
    every rank.  ``items``: a ``FrameItems`` (its arena is the send block: no stacking) or a list of ``(features,
    labels)``; an empty one is fine as long as some rank has frames.  Under RCCL the exchange -- and the result, unless
    ``out_device`` says otherwise -- lives on this process's GPU.  Without an initialised process group: the block."""
    if isinstance(items, FrameItems):
        local = items.features
    elif len(items) > 0:
        local = torch.stack([f for f, _ in items], dim=0)
    else:
        local = None
    if local is not None and local.shape[0] == 0 and local.ndim < 3:
        local = None
    return hdist.all_gather_ragged(local, group, out_device=out_device)
