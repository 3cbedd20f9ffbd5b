"""The file pipeline behind extract_features(): clip files in, feature files out, every stage overlapped.  _FilePipeline holds the
_Slots (cached per parameter set for the life of the process: pipeline_for), a _Run holds the state and the three stages of ONE run(),
ScalerSums carries compute_scaler's statistics out.  The switches live on salsa_amd.features; this module is handed what it needs."""
import logging
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import io as sio

_log = logging.getLogger('salsa_amd.features')

SLOT_CLIPS = 8     # clips per pipeline slot: small slots overlap read / copy / extract / copy / write sooner and pin 4x less host memory
                   # than 32-clip ones; the device does 8 x 60-s clips in ~0.45 ms, far below a slot's 8 ms of PCIe time
_STOP = object()


def _timed(fn, *args, **kw):
    t0 = time.perf_counter()
    fn(*args, **kw)
    return time.perf_counter() - t0


def pcm_to_planar(d_raw, code, d_out):
    """d_raw: a clip's place in a device slot holding the WAV file's data chunk ([N][4] samples of SALSA_PCM_* ``code``) -> d_out float32
    [4][N], on the current stream (salsa_pcm_to_planar)."""
    import ctypes as C
    import torch
    from . import _lib
    rc = _lib.load().salsa_pcm_to_planar(C.c_void_p(d_raw.data_ptr()), int(code), int(d_out.shape[0]), int(d_out.shape[1]),
                                         C.c_void_p(d_out.data_ptr()), C.c_void_p(torch.cuda.current_stream(d_out.device).cuda_stream))
    if rc != 0:
        raise RuntimeError('salsa_pcm_to_planar failed (%d): %s' % (rc, _lib.last_error()))


class ScalerSums:
    """compute_scaler's statistics (:204-262) taken from the features while they are on the device instead of reading every file back:
    ``sums`` float64 [2][4][F] device tensor (sum / sum of squares of the spectrogram channels over every frame extracted), ``n_frames``,
    and whether they are ``available`` (not after the serial loop or an empty split: compute_scaler reads the files then)."""

    def __init__(self):
        self.sums, self.n_frames, self.available = None, 0, True

    def add(self, partial_sums, n_frames):
        for s in partial_sums:
            if s is not None:
                self.sums = s.clone() if self.sums is None else self.sums + s
        self.n_frames += n_frames


class _Slot:
    """One batch on its way through the pipeline.  What lasts between runs: the extractor, the streams and the flat arrays, which
    only ever GROW (a tree of ragged clips used to re-pin its slots at every new length).  The rest describes the current batch."""

    def __init__(self, idx, ex, torch):
        self.idx, self.ex, self.torch = idx, ex, torch
        self.s_in, self.s_run, self.s_out = (torch.cuda.Stream(device=ex.device) for _ in range(3))
        self.f_h_in = self.f_d_in = self.f_d_out = self.f_h_out = None    # flat pinned (h) / device (d) arrays ...
        self.cap_in = self.cap_out = 0                                     # ... and their sizes in floats
        self.f_d_conv = None                # flat device array: clips uploaded as raw PCM are converted into it (sized on first use)
        self.shape = self.h_in = self.d_in = self.d_out = self.h_out = None    # (batch, n_samples) and the views of the flat arrays for it
        self.items, self.raw = [], []       # the batch: [(count, file name)]; per clip 0 = float32 samples in the slot, else its SALSA_PCM_* code
        self.done = None                    # event: the batch's features are in h_out

    def buffers(self, batch, n_samples):
        """Views of the slot's staging for (batch, n_samples)."""
        if self.shape == (batch, n_samples):
            return
        torch, ex = self.torch, self.ex
        shape = (batch, 4, n_samples) if ex.audio_layout == 'planar' else (batch, n_samples, 4)
        oshape = (batch,) + tuple(ex.output_shape(n_samples))
        n_in, n_out = int(np.prod(shape)), int(np.prod(oshape))
        if self.cap_in < n_in:
            self.f_h_in = torch.empty(n_in, dtype=torch.float32, pin_memory=True)
            self.f_d_in = torch.empty(n_in, dtype=torch.float32, device=ex.device)
            self.cap_in = n_in
        if self.cap_out < n_out:
            self.f_d_out = torch.empty(n_out, dtype=torch.float32, device=ex.device)
            self.f_h_out = torch.empty(n_out, dtype=torch.float32, pin_memory=True)
            self.cap_out = n_out
        self.h_in, self.d_in = self.f_h_in[:n_in].view(shape), self.f_d_in[:n_in].view(shape)
        self.d_out, self.h_out = self.f_d_out[:n_out].view(oshape), self.f_h_out[:n_out].view(oshape)
        self.shape = (batch, n_samples)


class _Run:
    """One run() of a pipeline: queues, stop flag, first error, stage timers, per-slot scaler sums and frame count.  _FilePipeline.run
    drops it when it returns or raises, so nothing of a run -- least of all a failed run's statistics -- can reach the next one."""

    def __init__(self, pipe, todo, audio_dir, feature_dir, fs, cap, raw_pcm, want_sums):
        self.pipe, self.todo, self.audio_dir, self.feature_dir, self.fs, self.cap = pipe, todo, audio_dir, feature_dir, fs, cap
        self.device, self.planar = pipe.ex.device, pipe.ex.audio_layout == 'planar'
        self.raw_pcm = raw_pcm and self.planar              # (the device conversion writes the planar layout)
        self.free, self.filled, self.inflight = queue.Queue(), queue.Queue(), queue.Queue()
        self.stop, self.error, self.batches, self.read_s, self.write_s = threading.Event(), None, 0, 0.0, 0.0
        self.wait = {'main_for_reader': 0.0, 'writer_for_device': 0.0, 'reader_for_slot': 0.0}
        self.sums, self.n_frames = ([None] * len(pipe.slots) if want_sums else None), 0    # float64 [2][4][F] per slot, on its own stream
        self.open = {}                      # reader: n_samples -> (slot being filled, [futures of its reads])
        self.pending = []                   # reader: closed (slot, futures) whose clips are still being read, in closing order
        for sl in pipe.slots:
            self.free.put(sl)

    def fail(self, e):
        """Record the first failure of any stage and tell every other stage to stop."""
        self.error = self.error or e
        self.stop.set()

    def take(self, q, waiting=None):
        """q.get() that gives up (returns _STOP) once any stage has failed: no stage may block forever on a queue whose producer is
        gone (a failed extract() or writer used to leave the reader in free.get() and run() in join())."""
        t0 = time.perf_counter()
        while True:
            try:
                got = q.get(timeout=0.05)
            except queue.Empty:
                if not self.stop.is_set():
                    continue
                got = _STOP
            if waiting:
                self.wait[waiting] += time.perf_counter() - t0
            return got

    def reader(self):
        """Stage 1, a thread: reads each clip's HEADER, gives it a place in a free slot's pinned input (one batch = clips of one length,
        in file order) and hands the decode to a pool of reader threads, which read STRAIGHT INTO that place."""
        pool = ThreadPoolExecutor(self.pipe.readers)
        try:
            self.pipe.torch.cuda.set_device(self.device)    # (a new thread starts on device 0)
            for count, fn in self.todo:
                if self.stop.is_set() or not self._place(pool, count, fn):
                    return
            for n in sorted(self.open, key=lambda k: self.open[k][0].items[0][0]):
                self._close(n)
            self._publish(0)
        except BaseException as e:                          # noqa: BLE001 - re-raised by run()
            self.fail(e)
        finally:
            pool.shutdown(wait=True)
            self.filled.put(None)

    def _place(self, pool, count, fn):
        """Issue the read of one clip into the open slot of its length; False if the run stopped while waiting for a slot."""
        path = os.path.join(self.audio_dir, fn)
        # a plain PCM / float WAV at the configured rate goes to the device AS IT IS ON DISK (decoding 16-bit clips on the host: 14 k audio-s/s)
        lay = sio.wav_pcm_layout(path, self.fs) if self.raw_pcm else None
        n_ch, n = (lay[1], lay[2]) if lay else sio.audio_shape(path, self.fs)     # header only
        assert n_ch == 4, '{}: expected a 4-channel clip'.format(fn)
        if n not in self.open:
            if len(self.open) >= self.pipe.depth - 2:       # never hold every slot half-filled: flush the fullest bucket
                self._close(max(self.open, key=lambda k: len(self.open[k][0].items)))
            sl = self.take(self.free, 'reader_for_slot')
            if sl is _STOP:
                return False
            sl.buffers(self.cap, n)
            sl.items, sl.raw = [], [0] * self.cap
            self.open[n] = (sl, [])
        sl, futs = self.open[n]
        place = sl.h_in.numpy()[len(sl.items)]
        if lay:
            sl.raw[len(sl.items)] = lay[0]
            nbytes = n * 4 * {1: 2, 2: 4, 3: 1, 4: 4}[lay[0]]
            futs.append(pool.submit(_timed, sio.read_raw_into, path, lay[3], place.reshape(-1).view(np.uint8)[:nbytes]))
        else:
            futs.append(pool.submit(_timed, sio.load_audio_into, path, self.fs, place, self.planar, device=self.device))
        sl.items.append((count, fn))
        if len(sl.items) == self.cap:
            self._close(n)
        return True

    def _close(self, n):
        self.pending.append(self.open.pop(n))
        self._publish(1)                                    # the next slot's reads are issued while this one's finish

    def _publish(self, keep):
        """Hand the oldest closed slots to the device stage once their reads have finished (never more than ``keep`` waiting)."""
        while self.pending and (len(self.pending) > keep or all(f.done() for f in self.pending[0][1])):
            sl, futs = self.pending.pop(0)
            for f in futs:
                self.read_s += f.result()                   # (re-raises a failed read here, in the reader thread)
            self.filled.put(sl)

    def issue(self):
        """Stage 2, the caller's thread: queues every filled slot's host->device copy, kernels and device->host copy on its streams (nothing blocks)."""
        try:
            while not self.stop.is_set():                   # (a failed stage: launch nothing more, not even what is already queued)
                sl = self.take(self.filled, 'main_for_reader')
                if sl is None or sl is _STOP:
                    break
                self._issue_slot(sl)
                self.inflight.put(sl)
                self.batches += 1
        except BaseException as e:                          # noqa: BLE001 - a failed copy / extract in THIS thread stops the others too
            self.fail(e)
        finally:
            self.inflight.put(None)                         # (the writer finishes what is in flight, or leaves at once after a failure)

    def _issue_slot(self, sl):
        torch, b = self.pipe.torch, len(sl.items)
        with torch.cuda.stream(sl.s_in):
            sl.d_in[:b].copy_(sl.h_in[:b], non_blocking=True)
        sl.s_run.wait_stream(sl.s_in)
        with torch.cuda.stream(sl.s_run):
            d_audio = sl.d_in
            if any(sl.raw[:b]):                             # raw file bytes in the slot: convert + de-interleave on the device
                if sl.f_d_conv is None or sl.f_d_conv.numel() < sl.cap_in:
                    sl.f_d_conv = torch.empty(sl.cap_in, dtype=torch.float32, device=self.device)
                d_audio = sl.f_d_conv[:sl.d_in.numel()].view(sl.d_in.shape)
                for k in range(b):
                    if sl.raw[k]:
                        pcm_to_planar(sl.d_in[k], sl.raw[k], d_audio[k])
                    else:
                        d_audio[k].copy_(sl.d_in[k], non_blocking=True)
            sl.ex.extract(d_audio[:b], out=sl.d_out[:b])
            if self.sums is not None:
                from .extractor import scaler_accumulate
                if self.sums[sl.idx] is None:
                    self.sums[sl.idx] = torch.zeros((2, 4, sl.d_out.shape[3]), dtype=torch.float64, device=self.device)
                scaler_accumulate(sl.d_out[:b], self.sums[sl.idx])
                self.n_frames += b * sl.d_out.shape[2]
        sl.s_out.wait_stream(sl.s_run)
        with torch.cuda.stream(sl.s_out):
            sl.h_out[:b].copy_(sl.d_out[:b], non_blocking=True)
            sl.done = torch.cuda.Event()
            sl.done.record(sl.s_out)

    def writer(self):
        """Stage 3, a thread: waits for each slot's event, writes its feature files from the pinned output with a pool, hands it back."""
        pool = ThreadPoolExecutor(self.pipe.writers)
        try:
            self.pipe.torch.cuda.set_device(self.device)
            while not self.stop.is_set():
                sl = self.take(self.inflight)
                if sl is None or sl is _STOP:
                    return
                self.wait['writer_for_device'] += _timed(sl.done.synchronize)
                t0, feats = time.perf_counter(), sl.h_out.numpy()
                def save(k):
                    count, fn = sl.items[k]
                    sio.save_arrays(os.path.join(self.feature_dir, sio.feature_name(fn)), feature=feats[k])
                    _log.debug('clip %d %s -> %s', count, fn, feats[k].shape)
                list(pool.map(save, range(len(sl.items))))
                self.write_s += time.perf_counter() - t0
                self.free.put(sl)
        except BaseException as e:                          # noqa: BLE001
            self.fail(e)
        finally:
            pool.shutdown(wait=True)


class _FilePipeline:
    """``depth`` slots, each with pinned host staging in both directions, device buffers, its own plan and its own copy-in / compute /
    copy-out streams, so the decode of batch i+2, the PCIe transfers and kernels of batch i+1 and the file writes of batch i run at the
    same time (the stages: _Run).  Between runs the pipeline holds only the slots' grown buffers, plans and streams."""

    def __init__(self, ex, depth=4, writers=None, readers=None):
        if depth < 3:                                       # (the reader keeps depth - 2 length buckets open: at least one)
            raise ValueError('_FilePipeline needs depth >= 3, got {}'.format(depth))
        import torch
        from .extractor import SalsaExtractor
        try:
            ncpu = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            ncpu = os.cpu_count() or 1
        # pools sized to the CPUs this process may use (ONE reader thread: 11 ms per 60-s clip = 5.3 k audio-s/s, the harness' whole bound)
        self.readers, self.writers = (int(n or max(1, min(8, ncpu // 2))) for n in (readers, writers))
        self.torch, self.depth = torch, depth
        self.slots = [_Slot(i, ex if i == 0 else SalsaExtractor(**ex.kwargs()), torch) for i in range(depth)]
        self.lock = threading.Lock()        # (the pipeline of a parameter set is shared by every call in the process: one run at a time)

    @property
    def ex(self):                           # slot 0's extractor is the caller's: every run copies its plan state to the other slots
        return self.slots[0].ex

    def adopt(self, ex):                    # ``ex`` (same parameters and device: pipeline_for's key) becomes slot 0's, and so the state source
        self.slots[0].ex = ex

    def run(self, todo, audio_dir, feature_dir, fs, batch_size, stats=None, scaler=None, raw_pcm=True, slot_clips=SLOT_CLIPS):
        """todo: [(count, file name)] in order.  Writes <feature_dir>/<feature_name(fn)> for every clip; the first exception of any stage
        stops the others and is re-raised here.  stats: a dict that receives the stage timers.  scaler: a ScalerSums that receives the run's
        statistics (salsa_scaler_accumulate on each slot's own stream into the slot's own sums, added in slot order at the end)."""
        torch, wall = self.torch, time.perf_counter()
        # the clones were built from the constructor arguments only: carry over the plan state attached since (a scaler, a schedule)
        for sl in self.slots[1:]:
            self.ex.copy_plan_state_to(sl.ex)
        cap = max(1, min(batch_size, slot_clips, len(todo)))    # clips per slot (batch_size is the caller's upper bound per device call)
        run = _Run(self, todo, audio_dir, feature_dir, fs, cap, raw_pcm, scaler is not None)
        tr, tw = threading.Thread(target=run.reader, daemon=True), threading.Thread(target=run.writer, daemon=True)
        tr.start(), tw.start()
        run.issue()
        tw.join()
        tr.join()
        if run.error or scaler is not None:                 # (after a failure in-flight device work may still touch the pinned slots)
            torch.cuda.synchronize(self.ex.device)
        if run.error:
            raise run.error
        if scaler is not None:
            scaler.add(run.sums, run.n_frames)
        if stats is not None:
            stats.update(batches=run.batches, read_s=run.read_s, write_s=run.write_s, wall=time.perf_counter() - wall, **run.wait)


_PIPELINES = {}


def pipeline_for(ex):
    """The file pipeline of extractors with these parameters on this device, built once per process: its plans, streams and -- above
    all -- its pinned host slots outlive an extract_features() call (pinning 6 GB of slots cost more than extracting a 64-clip tree).
    The caller's extractor becomes slot 0's; its post-construction state (scaler, schedule) is re-applied to every slot by run()."""
    key = (str(ex.device),) + tuple(sorted((k, str(v)) for k, v in ex.kwargs().items()))
    if key not in _PIPELINES:
        _PIPELINES[key] = _FilePipeline(ex)
    _PIPELINES[key].adopt(ex)
    return _PIPELINES[key]


def release_file_pipelines():
    """Drop the cached pipelines (pinned host slots, device buffers, plans)."""
    _PIPELINES.clear()
