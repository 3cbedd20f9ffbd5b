"""Test-time augmentation (TTA) and model ensembling around an inference forward.  The reference publishes
numbers for both ("FOA SALSA w/ TTA", the DCASE 2021 ensemble) but ships code for neither, so the definition is this project's:

  variants   the channel swaps of the training augmentation, enumerated: kind 'foa' has V = 16 (m[j] = bit j of v, four bits), 'mic'
             V = 8 (three bits), 'gcc' V = 4 (v = 0 no swap, v = 1, 2, 3 the one-hot m with bit v - 1 set: GccRandomSwapChannelMic acts
             on the first set bit only).  Variant 0 is the input itself.  x_v = augment.swap_channels_*(x, m), bit for bit.
  un-swap    a model fed x_v predicts S_m(d), S_m = augment.swap_targets(., m): its output is rotated back with S_m^-1
             (unswap_targets; every bit's step is its own inverse, so the steps run in reverse bit order; exact).  The event
             activities are not transformed.
  merge      the N = models x variants outputs are added in float32, models outer and variants in list order, starting from the
             first, and divided once by float(N) (correctly rounded).  prob and xyz alike; with output_format 'accdoa' the merged
             activity is nn_ops.accdoa_sed(merged xyz), not the mean of the lengths.

  multi      output_format 'multi_accdoa' holds three unordered tracks per class, so its forwards are merged only under
             track_merge='align' (tta_merge_multi): every slab is un-swapped, every slab after the first is
             permuted, (clip, frame, class) cell by cell, onto slab 0 by the candidate of least squared distance (ADPIT's six
             permutations and cost walk), then the same fixed-order sum and one division; the activities are the merged lengths.

CUDA float32 tensors go through salsa_nn_tta_variant / salsa_nn_tta_merge / salsa_nn_tta_merge_multi (csrc/tta.hip,
csrc/track_align.hip); CPU tensors, and everything under SALSA_HIP_TTA=0, through the torch operators."""
import ctypes as C
import os

import torch

from .. import _lib, augment

USE_HIP_TTA = os.environ.get('SALSA_HIP_TTA', '1') != '0'   # 0: both steps on the torch operators
KIND = {'foa': 1, 'mic': 2, 'gcc': 3}                      # include/salsa_nn.h (= _lib.BANK_RECIPE)
_V = {'foa': 16, 'mic': 8, 'gcc': 4}
_CHANNELS = {'foa': 7, 'mic': 7, 'gcc': 10}
MAX_VARIANTS = 16                                          # a call's variant list (csrc/tta.h)


def _kind(kind):
    if kind not in KIND:
        raise ValueError("kind must be 'foa', 'mic' or 'gcc', not {!r}".format(kind))
    return kind


def n_variants(kind):
    return _V[_kind(kind)]


def variant_bits(kind, v):
    """the swap bits m of variant v: a tuple of 4 (foa) or 3 (mic, gcc) ints in {0, 1}"""
    V = n_variants(kind)
    if not 0 <= int(v) < V:
        raise ValueError('variant %r of kind %s: there are %d' % (v, kind, V))
    v = int(v)
    if kind == 'gcc':
        return tuple(int(v == j + 1) for j in range(3))
    return tuple((v >> j) & 1 for j in range(4 if kind == 'foa' else 3))


def unswap_targets(y_doa, m, audio_format='foa', n_classes: int = 12):
    """The inverse of augment.swap_targets: y_doa (B, T_lab, 3 nc), m (B, >= 3 | 4) in {0, 1} -> new tensor with
    swap_targets(unswap_targets(y, m), m) == y == unswap_targets(swap_targets(y, m), m), bit for bit.  Branch-free like its
    counterpart (torch.where on the per-sample bits), any device.  The gcc kind's targets follow 'mic'."""
    nc = n_classes
    b = m.to(device=y_doa.device, dtype=torch.bool)[:, :, None, None]            # (B, bits, 1, 1)
    x, y, z = y_doa[:, :, :nc], y_doa[:, :, nc:2 * nc], y_doa[:, :, 2 * nc:]
    if audio_format == 'foa':                                                     # bits 3..1: negate z, y, x
        x, y, z = torch.where(b[:, 1], -x, x), torch.where(b[:, 2], -y, y), torch.where(b[:, 3], -z, z)
    else:
        y, z = torch.where(b[:, 2], -y, y), torch.where(b[:, 2], -z, z)          # bit 2: negate y and z
        x, y = torch.where(b[:, 1], -y, x), torch.where(b[:, 1], -x, y)          # bit 1: swap x and y, negate both
    x, y = torch.where(b[:, 0], y, x), torch.where(b[:, 0], x, y)                # bit 0: swap x and y, last
    return torch.cat([x, y, z], dim=2)


def _check_features(x, kind):
    if x.dim() != 4 or x.shape[1] != _CHANNELS[kind]:
        raise ValueError('the %s recipe takes features (B, %d, T, F), not %s' % (kind, _CHANNELS[kind], tuple(x.shape)))


def _hip_features(x):
    return USE_HIP_TTA and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 and augment._rows_contiguous(x)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def tta_variant(x, kind, v, out=None):
    """Variant v of the feature batch x (B, C, T, F), C = 7 (foa, mic) or 10 (gcc).  v = 0: x itself, no copy.  CUDA float32 x with
    dense (T, F) rows (time-cropped and batch-strided views included): one salsa_nn_tta_variant launch on the current stream, into
    ``out`` when given (dense float32 of x's shape, not x).  Anything else: augment.swap_channels_* (``out`` is not used)."""
    _check_features(x, _kind(kind))
    m = variant_bits(kind, v)
    if int(v) == 0:
        return x
    if _hip_features(x):
        if out is None:
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
            raise ValueError('out must be a dense float32 tensor of the shape and device of x')
        B, _, T, F = x.shape
        with torch.cuda.device(x.device):
            rc = _lib.load().salsa_nn_tta_variant(C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), C.c_void_p(out.data_ptr()), B, T, F,
                                                  KIND[kind], int(v), _stream(x))
        if rc:
            raise RuntimeError('salsa_nn_tta_variant failed: ' + _lib.last_error())
        return out
    mb = torch.tensor(m, dtype=torch.long).expand(x.shape[0], -1)
    if kind == 'gcc':
        return augment.swap_channels_gcc(x, mb)
    swap = augment.swap_channels_foa if kind == 'foa' else augment.swap_channels_mic
    return swap(x, x.new_zeros((x.shape[0], 1, 3)), mb.to(x.device), 1)[0]


def _ids(kind, variant_ids):
    ids = [int(v) for v in variant_ids]
    V = n_variants(kind)
    if not 1 <= len(ids) <= MAX_VARIANTS or any(not 0 <= v < V for v in ids):
        raise ValueError('variant ids %s: 1 to %d ids in [0, %d) for kind %s' % (ids, MAX_VARIANTS, V, kind))
    return ids


def _merge_torch(prob_slab, xyz_slab, n_models, ids, kind, n_classes):
    """the merge rules with torch operators: un-swap, sequential float32 adds in slab order from the first slab, one true division
    (by a TENSOR: torch multiplies by the reciprocal when the divisor is a Python number)"""
    fmt = 'foa' if kind == 'foa' else 'mic'
    B = prob_slab.shape[1]
    p = d = None
    n = 0
    for _ in range(n_models):
        for v in ids:
            m = torch.tensor(variant_bits(kind, v), dtype=torch.long).expand(B, -1)
            dv = unswap_targets(xyz_slab[n], m, fmt, n_classes)
            p, d = (prob_slab[n], dv) if n == 0 else (p + prob_slab[n], d + dv)
            n += 1
    div = torch.full((), float(n), dtype=torch.float32, device=prob_slab.device)
    return p / div, d / div


def tta_merge(prob_slab, xyz_slab, n_models, variant_ids, kind, n_classes: int = 12, _ids_c=None):
    """prob_slab (N, B, L, nc), xyz_slab (N, B, L, 3 nc) float32, N = n_models * len(variant_ids), slab model * len(variant_ids) + i
    = the forward output for variant variant_ids[i] -> merged (prob (B, L, nc), xyz (B, L, 3 nc)) by the module's rules.  CUDA: one
    salsa_nn_tta_merge launch on the current stream; CPU (and SALSA_HIP_TTA=0): the torch restatement of the same rules."""
    ids = _ids(_kind(kind), variant_ids)
    N = n_models * len(ids)
    if n_models < 1 or prob_slab.dim() != 4 or xyz_slab.dim() != 4 or prob_slab.shape[0] != N or xyz_slab.shape[0] != N or \
            prob_slab.shape[1:3] != xyz_slab.shape[1:3] or prob_slab.shape[3] != n_classes or xyz_slab.shape[3] != 3 * n_classes:
        raise ValueError('slabs %s / %s for %d models x %d variants of %d classes' % (tuple(prob_slab.shape), tuple(xyz_slab.shape),
                                                                                     n_models, len(ids), n_classes))
    if not (USE_HIP_TTA and prob_slab.is_cuda and xyz_slab.is_cuda and prob_slab.numel() > 0):
        return _merge_torch(prob_slab.float(), xyz_slab.float(), n_models, ids, kind, n_classes)
    if prob_slab.dtype != torch.float32 or xyz_slab.dtype != torch.float32 or not prob_slab.is_contiguous() or not xyz_slab.is_contiguous():
        raise ValueError('the slabs are dense float32 tensors')
    _, B, L, _ = prob_slab.shape
    prob = torch.empty((B, L, n_classes), dtype=torch.float32, device=prob_slab.device)
    xyz = torch.empty((B, L, 3 * n_classes), dtype=torch.float32, device=prob_slab.device)
    ids_c = _ids_c if _ids_c is not None else (C.c_int * len(ids))(*ids)
    with torch.cuda.device(prob_slab.device):
        rc = _lib.load().salsa_nn_tta_merge(C.c_void_p(prob_slab.data_ptr()), C.c_void_p(xyz_slab.data_ptr()), n_models, ids_c, len(ids),
                                            KIND[kind], B, L, n_classes, C.c_void_p(prob.data_ptr()), C.c_void_p(xyz.data_ptr()),
                                            _stream(prob_slab))
    if rc:
        raise RuntimeError('salsa_nn_tta_merge failed: ' + _lib.last_error())
    return prob, xyz


def _check_track_merge(track_merge, output_format):
    if track_merge not in (None, 'align'):
        raise ValueError("track_merge must be None or 'align', not {!r}".format(track_merge))
    if track_merge == 'align' and output_format != 'multi_accdoa':
        raise ValueError("track_merge='align' aligns the tracks of output_format 'multi_accdoa'; %r has none" % (output_format,))


def _align_torch(R, V):
    """csrc/track_align.h's align_cell on (B, L, axis, track, C) float32 tensors -> candidates (B, L, C) int64: sequential float64
    adds, tracks outer and axes inner, and an explicit strict-less walk over the six candidates (argmin's NaN rule differs)"""
    from .postprocess import TRACK_PERMS
    R, V = R.double(), V.double()
    chosen = best = None
    for cand, perm in enumerate(TRACK_PERMS):
        e = torch.zeros(R.shape[:2] + R.shape[4:], dtype=torch.float64, device=R.device)
        for n in range(3):
            for a in range(3):
                d = R[:, :, a, n] - V[:, :, a, perm[n]]
                e = e + d * d
        if cand == 0:
            best, chosen = e, torch.zeros(e.shape, dtype=torch.long, device=R.device)
        else:
            less = e < best
            best, chosen = torch.where(less, e, best), torch.where(less, torch.full_like(chosen, cand), chosen)
    return chosen


def _merge_multi_torch(xyz_slab, n_models, ids, kind, n_classes):
    """tta_merge_multi's rules with torch operators: un-swap (per column, so per track), align every later slab to slab 0,
    sequential float32 adds in slab order from slab 0, one true division by a tensor -> (xyz (B, L, 9 C), perm (N, B, L, C) int32)"""
    from .postprocess import TRACK_PERMS
    fmt = 'foa' if kind == 'foa' else 'mic'
    N, B, L, _ = xyz_slab.shape
    table = torch.tensor(TRACK_PERMS, dtype=torch.long, device=xyz_slab.device)
    perm = torch.zeros((N, B, L, n_classes), dtype=torch.int32, device=xyz_slab.device)
    R = acc = None
    for k in range(N):
        m = torch.tensor(variant_bits(kind, ids[k % len(ids)]), dtype=torch.long).expand(B, -1)
        V = unswap_targets(xyz_slab[k], m, fmt, 3 * n_classes).reshape(B, L, 3, 3, n_classes)       # (B, L, axis, track, C)
        if k == 0:
            R = acc = V
            continue
        cand = _align_torch(R, V)
        perm[k] = cand.to(torch.int32)
        src = table[cand].permute(0, 1, 3, 2)[:, :, None].expand(B, L, 3, 3, n_classes)             # the source of (axis, track n, c)
        acc = acc + torch.gather(V, 3, src)
    div = torch.full((), float(N), dtype=torch.float32, device=xyz_slab.device)
    return (acc / div).reshape(B, L, 9 * n_classes), perm


def tta_merge_multi(xyz_slab, n_models, variant_ids, kind, n_classes: int = 12, return_perm: bool = False, _ids_c=None):
    """The merge of output_format 'multi_accdoa' under track_merge='align' (DESIGN.md section 9u): xyz_slab (N, B, L, 9 C) float32,
    N = n_models * len(variant_ids) ordered as tta_merge's, C = n_classes REAL classes -> (act (B, L, 3 C), xyz (B, L, 9 C)), and with
    return_perm the chosen candidates (N, B, L, C) int32 (postprocess.TRACK_PERMS[cand][n] = the track of the slab that was added to
    track n; 0 for slab 0).  Slab 0 is the anchor; every later slab is aligned to it alone.  act = nn_ops.accdoa_sed(xyz, 3 C).  CUDA:
    one salsa_nn_tta_merge_multi launch on the current stream; CPU (and SALSA_HIP_TTA=0): the torch restatement, the same bits."""
    ids = _ids(_kind(kind), variant_ids)
    N = n_models * len(ids)
    if n_models < 1 or xyz_slab.dim() != 4 or xyz_slab.shape[0] != N or xyz_slab.shape[3] != 9 * n_classes:
        raise ValueError('slab %s for %d models x %d variants of %d classes with three tracks' % (tuple(xyz_slab.shape), n_models, len(ids), n_classes))
    if not (USE_HIP_TTA and xyz_slab.is_cuda and xyz_slab.numel() > 0):
        from .nn_ops import accdoa_sed
        xyz, perm = _merge_multi_torch(xyz_slab.float(), n_models, ids, kind, n_classes)
        act = accdoa_sed(xyz, 3 * n_classes)
        return (act, xyz, perm) if return_perm else (act, xyz)
    if xyz_slab.dtype != torch.float32 or not xyz_slab.is_contiguous():
        raise ValueError('the slab is a dense float32 tensor')
    _, B, L, _ = xyz_slab.shape
    dev = xyz_slab.device
    act = torch.empty((B, L, 3 * n_classes), dtype=torch.float32, device=dev)
    xyz = torch.empty((B, L, 9 * n_classes), dtype=torch.float32, device=dev)
    perm = torch.empty((N, B, L, n_classes), dtype=torch.int32, device=dev) if return_perm else None
    ids_c = _ids_c if _ids_c is not None else (C.c_int * len(ids))(*ids)
    with torch.cuda.device(dev):
        rc = _lib.load().salsa_nn_tta_merge_multi(C.c_void_p(xyz_slab.data_ptr()), n_models, ids_c, len(ids), KIND[kind], B, L, n_classes,
                                                  C.c_void_p(xyz.data_ptr()), C.c_void_p(act.data_ptr()),
                                                  C.c_void_p(perm.data_ptr()) if return_perm else None, _stream(xyz_slab))
    if rc:
        raise RuntimeError('salsa_nn_tta_merge_multi failed: ' + _lib.last_error())
    return (act, xyz, perm) if return_perm else (act, xyz)


class TtaForward:
    """A forward that runs ``forwards`` on every selected variant of its input and returns the merged (prob, xyz), with the shapes
    and dtypes of one forward call -- so it goes wherever a forward goes (infer_pipelined, with chunks, either decode, scoring,
    sharding).  forwards: one callable or a sequence of callables with Trainer.infer's signature (several: an ensemble).
    variants: 'all'; None or () for the identity only (a plain ensemble); or a list of at most 16 ids, merged in list order.
    A variant is formed once and fed to every model.  One variant buffer and one pair of slabs are kept and reused across calls
    (reallocated only to grow); every forward output is COPIED into its slab, so a forward may reuse its output storage.  All
    work is issued on the current stream; nothing waits for the device.  The variant list is fixed at construction and travels
    to the merge kernel in its arguments.

    output_format 'multi_accdoa' is refused unless track_merge='align': then the forwards return the track activities (b, frames,
    3 C) and xyz (b, frames, 9 C) of n_classes = C real classes, only an xyz slab is kept, the tracks are aligned cell by cell before
    the sum (tta_merge_multi) and the result is (accdoa_sed(xyz, 3 C), xyz)."""

    def __init__(self, forwards, audio_format, feature_type='salsa', variants='all', n_classes: int = 12,
                 output_format: str = 'reg_xyz', track_merge=None):
        self.kind = augment.recipe(audio_format, feature_type)[0]
        self.forwards = [forwards] if callable(forwards) else list(forwards)
        if not self.forwards or not all(callable(f) for f in self.forwards):
            raise ValueError('forwards: one callable or a non-empty sequence of callables')
        if output_format not in ('reg_xyz', 'accdoa', 'multi_accdoa'):
            raise ValueError('invalid output_format %r' % (output_format,))
        _check_track_merge(track_merge, output_format)
        if output_format == 'multi_accdoa' and track_merge is None:
            raise ValueError("output_format 'multi_accdoa' has no test-time augmentation by default: the track order differs between "
                             "forwards, so the variants cannot be averaged track by track; track_merge='align' aligns them first "
                             '(DESIGN.md sections 9i, 9u)')
        if isinstance(variants, str):
            if variants != 'all':
                raise ValueError("variants: 'all', None, () or a list of ids, not {!r}".format(variants))
            variants = range(n_variants(self.kind))
        elif variants is None or len(variants) == 0:
            variants = (0,)
        self.variant_ids = _ids(self.kind, variants)
        self._ids_c = (C.c_int * len(self.variant_ids))(*self.variant_ids)
        self.n_classes, self.output_format, self.track_merge = n_classes, output_format, track_merge
        self._buf = self._prob = self._xyz = None

    @staticmethod
    def _grown(buf, numel, device):
        if buf is None or buf.numel() < numel or buf.device != device:
            buf = torch.empty(numel, dtype=torch.float32, device=device)
        return buf

    def _variant(self, x, v):
        if v == 0 or not _hip_features(x):
            return tta_variant(x, self.kind, v)
        self._buf = self._grown(self._buf, x.numel(), x.device)
        return tta_variant(x, self.kind, v, out=self._buf[:x.numel()].view(x.shape))

    def __call__(self, features):
        _check_features(features, self.kind)
        nv, nc = len(self.variant_ids), self.n_classes
        N = len(self.forwards) * nv
        multi = self.output_format == 'multi_accdoa'
        w = 3 if multi else 1                                                # columns per real class: the tracks
        prob_slab = xyz_slab = p = d = None
        for vi, v in enumerate(self.variant_ids):
            xv = self._variant(features, v)
            for mi, forward in enumerate(self.forwards):
                p, d = forward(xv)
                if prob_slab is None:
                    if p.dim() != 3 or d.dim() != 3 or p.shape[2] != w * nc or d.shape[2] != 3 * w * nc or p.shape[:2] != d.shape[:2]:
                        raise ValueError('forward gave %s / %s, expected (b, frames, %d) / (b, frames, %d)'
                                         % (tuple(p.shape), tuple(d.shape), w * nc, 3 * w * nc))
                    if not multi:
                        self._prob = self._grown(self._prob, N * p.numel(), p.device)
                        prob_slab = self._prob[:N * p.numel()].view((N,) + tuple(p.shape))
                    self._xyz = self._grown(self._xyz, N * d.numel(), d.device)
                    xyz_slab = self._xyz[:N * d.numel()].view((N,) + tuple(d.shape))
                if not multi:
                    prob_slab[mi * nv + vi].copy_(p.detach())
                xyz_slab[mi * nv + vi].copy_(d.detach())
        if multi:
            act, xyz = tta_merge_multi(xyz_slab, len(self.forwards), self.variant_ids, self.kind, nc, _ids_c=self._ids_c)
            return act.to(p.dtype), xyz.to(d.dtype)
        prob, xyz = tta_merge(prob_slab, xyz_slab, len(self.forwards), self.variant_ids, self.kind, nc, _ids_c=self._ids_c)
        if self.output_format == 'accdoa':
            from .nn_ops import accdoa_sed
            prob = accdoa_sed(xyz, nc)
        return prob.to(p.dtype), xyz.to(d.dtype)


def wrap_forward(forward, tta, n_classes: int = 12, output_format: str = 'reg_xyz', track_merge=None):
    """the ``tta=`` keyword of infer_pipelined / validate / fit: None -> forward; a TtaForward -> itself (it carries its own
    forwards; with track_merge='align' it must have been built with it); an (audio_format, feature_type) pair ->
    TtaForward(forward, *pair) over all variants"""
    if tta is None:
        return forward
    if isinstance(tta, TtaForward):
        if track_merge == 'align' and tta.track_merge != 'align':
            raise ValueError("track_merge='align' with a ready TtaForward that was built without it")
        return tta
    audio_format, feature_type = tta
    return TtaForward(forward, audio_format, feature_type, n_classes=n_classes, output_format=output_format, track_merge=track_merge)
