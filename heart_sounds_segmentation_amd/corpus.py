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
All three builds below are fed by ONE such pipeline, ``CorpusBuilder._pipeline``: it owns the staging buffers, the three streams and
the events that say when a staging buffer or a half of the device ring may be overwritten.  A build hands it the groups, the arena
rows each group owns, the pointers to pack and its own launches for one group; nothing else differs between them.

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

import math
from collections.abc import Sequence as _SequenceABC
from typing import Callable, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
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


class _Group(NamedTuple):
    """What a build's launches are told about a group: recordings ``a:b`` of the list, rows ``r0:r1`` of the feature arena."""
    a: int
    b: int
    r0: int
    r1: int


def _host_f32(ts) -> Tuple[list, np.ndarray]:
    """Every tensor as contiguous host float32 (the tensor itself where it already is one), and the array of their addresses for
    ``_lib.pack_recordings``.  The caller keeps the list alive while the addresses are in use."""
    held = [t if (t.dtype == torch.float32 and t.is_contiguous() and not t.is_cuda) else t.detach().to("cpu", torch.float32).contiguous()
            for t in ts]                                  # (device recordings are staged through the host like the rest: rare)
    return held, np.asarray([t.data_ptr() for t in held], dtype=np.uint64)


def _sample_groups(lens_np: np.ndarray, max_samples: int) -> List[Tuple[int, int]]:
    """Groups ``(a, b)`` of consecutive recordings of at most ``max_samples`` samples (a longer recording is a group of its own)."""
    groups: List[Tuple[int, int]] = []
    g0, acc = 0, 0
    for i, T in enumerate(lens_np.tolist()):
        if acc > 0 and acc + T > max_samples:
            groups.append((g0, i))
            g0, acc = i, 0
        acc += T
    groups.append((g0, len(lens_np)))
    return groups


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
        self._bufs = None

    def _staging(self) -> dict:
        """The streams, the events and every staging buffer made so far (``_buf``), kept between calls."""
        if self._bufs is None:
            dev = self.dev
            self._bufs = {"up": torch.cuda.Stream(dev), "down": torch.cuda.Stream(dev),
                          "up_done": [torch.cuda.Event() for _ in range(2)], "used": [torch.cuda.Event() for _ in range(2)],
                          "ring_free": [torch.cuda.Event() for _ in range(2)]}
        return self._bufs

    def _buf(self, key: str, numel: int, dtype: torch.dtype = torch.float32, pinned: bool = False, count: int = 2) -> List[torch.Tensor]:
        """``count`` flat staging buffers ``key`` of at least ``numel`` elements, on the device or in pinned host memory.  They only
        grow, and their capacity is their own ``numel()``."""
        B = self._staging()
        cur = B.get(key)
        if cur is None or cur[0].numel() < numel or cur[0].dtype != dtype:
            where = {"pin_memory": True} if pinned else {"device": self.dev}
            cur = B[key] = [torch.empty(numel, dtype=dtype, **where) for _ in range(count)]
        return cur

    def _arena(self, shape: Tuple[int, ...], dtype: torch.dtype, keep_on_device: bool) -> torch.Tensor:
        """A feature arena: on the device, else in pinned host memory (``pin_host``), else pageable."""
        if keep_on_device:
            return torch.empty(shape, dtype=dtype, device=self.dev)
        try:
            return torch.empty(shape, dtype=dtype, pin_memory=bool(self.pin_host and shape[0] > 0))
        except RuntimeError:                              # page-locking that much memory can be refused: pageable then
            return torch.empty(shape, dtype=dtype)

    def _pipeline(self, groups: List[Tuple[int, int]], rows: np.ndarray, ptrs_np: np.ndarray, lens_np: np.ndarray,
                  feats: torch.Tensor, keep_on_device: bool, launch: Callable, tracks_np: Optional[np.ndarray] = None,
                  frame: Optional[Tuple[int, int]] = None, after: Optional[Callable] = None) -> None:
        """The double-buffered feed of every build.  ``groups``: ``(a, b)`` ranges of recordings (at least one); the samples of a
        group are those of its recordings (``lens_np``, addresses ``ptrs_np``), its rows of ``feats`` are ``rows[a]:rows[b]``.
        ``tracks_np``: addresses of label tracks of the same lengths, uploaded beside the samples.  ``frame``: the ``(stride,
        frame_len)`` of a framed build, whose frame starts are uploaded too (one start per arena row); None for whole recordings.

        Per group, ``launch(g, x, starts, tracks, dst)`` enqueues the build's work on the current stream: ``g`` a ``_Group``, ``x`` the
        packed samples on the device, ``starts`` the frame starts (None unless ``frame``), ``tracks`` the packed label tracks (None
        unless ``tracks_np``), ``dst`` the group's rows of the arena (``keep_on_device``) or a half of the device ring viewed to
        their shape, from which they are copied to the host arena on a third stream.  ``after(g)`` is host work of the group that
        overlaps its launches; it runs once the NEXT group's packing and upload are under way, so that it never delays them."""
        fsst, dev = self.fsst, self.dev
        stride, frame_len = frame if frame is not None else _lib.WHOLE_RECORDINGS
        pos_np = np.concatenate([[0], np.cumsum(lens_np)])
        item = tuple(feats.shape[1:])                    # one arena row: (C,) or (item_len, C)
        per_row = math.prod(item)
        gs = [_Group(a, b, int(rows[a]), int(rows[b])) for a, b in groups]
        sizes = [int(pos_np[g.b] - pos_np[g.a]) for g in gs]                         # samples of each group
        counts = [(g.r1 - g.r0) if frame is not None else (g.b - g.a) for g in gs]   # starts the pack call writes for it
        B = self._staging()
        stage_h, stage_d = self._buf("stage_h", max(sizes), pinned=True), self._buf("stage_d", max(sizes))
        if frame is not None:
            start_h, start_d = self._buf("start_h", max(counts), torch.int64, pinned=True), self._buf("start_d", max(counts), torch.int64)
        if tracks_np is not None:
            lab_h, lab_d = self._buf("lab_h", max(sizes), pinned=True), self._buf("lab_d", max(sizes))
        if not keep_on_device:                           # ONE kind of device ring: two flat halves, viewed per group
            ring = self._buf("ring", max(g.r1 - g.r0 for g in gs) * per_row, feats.dtype)
        aside = np.empty(max(counts), dtype=np.int64)    # starts that nobody reads: of whole recordings, of label tracks
        main, up, down = torch.cuda.current_stream(dev), B["up"], B["down"]
        up_done, used, ring_free = B["up_done"], B["used"], B["ring_free"]
        up.wait_stream(main)                             # (the staging buffers may still be read by an earlier call's work)

        # the host side of a group is ONE native call (hssfsst_pack_recordings: threaded copies into the pinned staging
        # buffer + the frame starts): per recording Python does nothing but hand over a pointer.  (Per-recording copy_ /
        # numpy calls were 0.29 ms per recording: 115 k windows/s however fast the device is.)
        def pack(gi: int) -> None:
            """Host side of group gi: recordings (and label tracks) back to back into pinned staging, frame starts; upload on `up`."""
            g, buf, n, ns = gs[gi], gi & 1, sizes[gi], counts[gi]
            if gi >= 2:
                used[buf].synchronize()                  # the launches of group gi - 2 no longer read this staging pair
            starts = start_h[buf].numpy() if frame is not None else aside[:ns]
            _lib.pack_recordings(ptrs_np[g.a:g.b], lens_np[g.a:g.b], stage_h[buf], starts, ns, stride, frame_len)
            if tracks_np is not None:
                _lib.pack_recordings(tracks_np[g.a:g.b], lens_np[g.a:g.b], lab_h[buf], aside[:ns], ns, stride, frame_len)
            with torch.cuda.stream(up):
                stage_d[buf][:n].copy_(stage_h[buf][:n], non_blocking=True)
                if frame is not None:
                    start_d[buf][:ns].copy_(start_h[buf][:ns], non_blocking=True)
                if tracks_np is not None:
                    lab_d[buf][:n].copy_(lab_h[buf][:n], non_blocking=True)
                up_done[buf].record(up)

        pack(0)
        for gi, g in enumerate(gs):
            buf, n, ns = gi & 1, sizes[gi], counts[gi]
            main.wait_event(up_done[buf])
            if keep_on_device:
                dst = feats[g.r0:g.r1]
            else:
                if gi >= 2:
                    main.wait_event(ring_free[buf])      # the copy of group gi - 2 has left this half of the ring
                dst = ring[buf][:(g.r1 - g.r0) * per_row].view((g.r1 - g.r0,) + item)
            launch(g, stage_d[buf][:n], start_d[buf][:ns] if frame is not None else None,
                   lab_d[buf][:n] if tracks_np is not None else None, dst)
            used[buf].record(main)
            if not keep_on_device:
                down.wait_stream(main)
                with torch.cuda.stream(down):
                    feats[g.r0:g.r1].copy_(dst, non_blocking=True)
                    ring_free[buf].record(down)
            if gi + 1 < len(gs):
                pack(gi + 1)                             # host packing + upload of the next group overlap these launches
            if after is not None:
                after(g)                                 # (host work, also overlapped)
        if not keep_on_device:
            down.synchronize()
        main.synchronize()
        fsst.check()

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
        feats = self._arena((total, C), fdt, keep_on_device)
        items = RecordingItems(RaggedFeatures(feats, offsets, K, False), ys)
        if total == 0:
            return items
        held, ptrs_np = _host_f32(xs)                   # (held: what the addresses point to, alive until the pipeline is through)

        def launch(g, x, starts, tracks, dst):
            fsst.ragged(x, lengths=lens_np[g.a:g.b], out=dst)

        # (a recording's rows of the arena are its samples)
        self._pipeline(_sample_groups(lens_np, max_samples), offsets.numpy(), ptrs_np, lens_np, feats, keep_on_device, launch)
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
        feats = self._arena((count, num, C), fdt, keep_on_device)
        if count == 0:
            return FrameItems(feats, None)
        groups = _sample_groups(lens_np, max_samples)
        rs_d = self._buf("rs_d", max(b - a for a, b in groups) * num, count=1)[0]     # a group's resampled recordings
        lab_d = torch.empty((count, num), dtype=torch.int64, device=dev) if have_labels else None
        held, ptrs_np = _host_f32(xs)
        # the label tracks as given (no shift), exact in float32, packed like the signals
        held_y, yptrs_np = _host_f32(ys) if have_labels else (None, None)

        def launch(g, x, starts, tracks, dst):
            rs = rs_d[:(g.b - g.a) * num].view(g.b - g.a, num)
            rsm.ragged(x, lengths=lens_np[g.a:g.b], out=rs)
            fsst.batch(rs, out=dst)
            if tracks is not None:
                rsm.ragged(tracks, lengths=lens_np[g.a:g.b], labels=True, out=lab_d[g.a:g.b])

        self._pipeline(groups, np.arange(count + 1), ptrs_np, lens_np, feats, keep_on_device, launch, tracks_np=yptrs_np)
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
        feats = out if out is not None else self._arena(shape, fdt, keep_on_device)
        if total == 0:
            if have_labels and rsm is not None:
                labels = torch.empty((0, out_len), dtype=torch.int64)
            return FrameItems(feats, labels)
        fr_np = np.concatenate([[0], np.cumsum(nfr_np)])  # a recording's rows of the arena are its frames
        dev_labels = have_labels and rsm is not None     # labels resampled on the device: (total, num) device arena, copied once
        lab_d = torch.empty((total, out_len), dtype=torch.int64, device=dev) if dev_labels else None
        if rsm is not None:                              # a group's resampled frames
            rs_d = self._buf("rs_d", max(int(fr_np[b] - fr_np[a]) for a, b in groups) * out_len, count=1)[0]
        held, ptrs_np = _host_f32([x for x, _ in recs])
        # the label tracks (y - 1), exact in float32, packed like the signals
        held_y, yptrs_np = _host_f32([y.reshape(-1) - 1 for _, y in recs]) if dev_labels else (None, None)

        def launch(g, x, starts, tracks, dst):
            if rsm is None:
                fsst.frames(x, starts, frame_len, out=dst)
            else:
                nf = g.r1 - g.r0
                rs = rs_d[:nf * out_len].view(nf, out_len)
                rsm.frames(x, starts, frame_len, out=rs)
                fsst.batch(rs, out=dst)
                if tracks is not None:
                    rsm.frames(tracks, starts, frame_len, labels=True, out=lab_d[g.r0:g.r1])

        self._pipeline(groups, fr_np, ptrs_np, lens_np, feats, keep_on_device, launch, tracks_np=yptrs_np, frame=(stride, frame_len),
                       after=(lambda g: fill_labels(g.a, g.b, g.r0)) if labels is not None else None)
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
