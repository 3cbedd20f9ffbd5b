"""SELD CRNN with the reference's architecture and initialisation (models/encoders.py:26-56 PannResNet22,
models/model_utils.py:187-228 ConvBlock, :312-367 basic block, :429-500 ResNet, models/decoders.py:13-154 SeldDecoder
with decoder_type='bigru', freq_pool='avg', decoder_size=256 -- experiments/configs/seld.yml:25-32 -- by default;
decoder_type 'gru' | 'lstm' | 'bilstm' and freq_pool 'max' | 'avg_max' are built too, 'transformer' is refused).

Shapes for an 8-s training chunk (7,640,200): stem (64,320,100) -> stage1 (64,320,100) -> stage2 (128,160,50) ->
stage3 (256,80,25) -> stage4 (512,40,12) -> mean over frequency (40,512) -> BiGRU (40,512) -> SED logits (40,12) and
xyz (40,36).  14.11 M parameters (11.21 M encoder + 2.90 M decoder)."""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .nn_ops import (BatchNormAct2d, Conv1x1, Conv3x3, ConvFilterBank, avg_pool2x2, conv1x1, conv_bn_act, folded_shortcut, freq_mean_sequence,
                     freq_pool_sequence, invalidate_conv_caches, new_backward_generation, stack_groups)


GRU_FP32 = os.environ.get('SALSA_GRU_FP32', '1') == '1'
FUSED_GRU = os.environ.get('SALSA_FUSED_GRU', '1') == '1'
BATCHED_HEADS = os.environ.get('SALSA_BATCHED_HEADS', '1') == '1'   # the four FC heads as one batch of four (Decoder._heads_batched)


def _xavier(layer):
    nn.init.xavier_uniform_(layer.weight)
    if getattr(layer, 'bias', None) is not None:
        layer.bias.data.zero_()
    return layer


def _conv(cin, cout, k):
    cls = Conv3x3 if k == 3 else Conv1x1 if k == 1 else nn.Conv2d                     # same parameters / state_dict; 64 -> 64 runs on the MFMA kernel
    return _xavier(cls(cin, cout, kernel_size=k, stride=1, padding=k // 2, bias=False))


class Stem(nn.Module):
    """two 3x3 conv + BN + ReLU, then 2x2 average pool (model_utils.py:187-228 with pool_type='avg')"""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1, self.bn1 = _conv(cin, cout, 3), BatchNormAct2d(cout)
        self.conv2, self.bn2 = _conv(cout, cout, 3), BatchNormAct2d(cout)

    def forward(self, x):
        x = conv_bn_act(self.conv1, self.bn1, x)
        return conv_bn_act(self.conv2, self.bn2, x, pool=True)                # ... -> 2x2 average pool


class ResBlock(nn.Module):
    """basic residual block; stride 2 is an average pool followed by stride-1 convs; dropout 0.1 after the first ReLU;
    the last BN starts at zero (zero_init_residual) -- model_utils.py:312-367."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.stride, self.dropout_p = stride, 0.1
        # set by the Encoder: this block's output is only ever read by the NEXT block's stride-2 average pool, so the pool is
        # taken here, fused into the last BatchNorm + add + ReLU (pool_out), and the next block skips its own (pre_pooled)
        self.pool_out, self.pre_pooled = False, False
        self.conv1, self.bn1 = _conv(cin, cout, 3), BatchNormAct2d(cout)
        self.conv2, self.bn2 = _conv(cout, cout, 3), BatchNormAct2d(cout)
        nn.init.zeros_(self.bn2.weight)
        self.short_conv, self.short_bn = None, None
        if stride != 1 or cin != cout:                      # 1x1 conv + BN shortcut (after the pool when strided)
            self.short_conv, self.short_bn = _conv(cin, cout, 1), BatchNormAct2d(cout)

    def forward(self, x):
        y = avg_pool2x2(x) if (self.stride == 2 and not self.pre_pooled) else x
        # dropout(relu(bn1(conv1(y)))), training only; ys is y for the shortcut branch (in training routed through conv1's
        # autograd node: the branch's gradient is added inside conv1's data-gradient kernel, not by a separate pass)
        out, ys = conv_bn_act(self.conv1, self.bn1, y, dropout_p=self.dropout_p, skip=True)
        if self.short_conv is not None:
            folded = folded_shortcut(self.short_conv, self.short_bn, ys)      # eval: BatchNorm folded into the 1x1 GEMM, its shift
            if folded is not None:                                            # added by conv2's epilogue with the residual
                return conv_bn_act(self.conv2, self.bn2, out, residual=folded[0], pool=self.pool_out, residual_shift=folded[1])
        sc = self.short_bn(conv1x1(self.short_conv, ys)) if self.short_conv is not None else ys
        return conv_bn_act(self.conv2, self.bn2, out, residual=sc, pool=self.pool_out)   # relu(bn2(conv2(out)) + shortcut) [-> pool]


class Encoder(nn.Module):
    """PANN ResNet22-style: stem + 4 stages x 2 blocks (64/128/256/512); time and frequency /16 (encoders.py:26-56)."""
    time_downsample_ratio = 16
    n_output_channels = 512

    def __init__(self, n_input_channels=7, p_dropout=0.0):
        super().__init__()
        self.p_dropout = p_dropout
        self.stem = Stem(n_input_channels, 64)
        blocks, cin = [], 64
        for cout, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
            blocks += [ResBlock(cin, cout, stride), ResBlock(cout, cout, 1)]
            cin = cout
        for prev, nxt in zip(blocks[:-1], blocks[1:]):
            if nxt.stride == 2:
                prev.pool_out, nxt.pre_pooled = True, True
        self.stages = nn.Sequential(*blocks)
        # one kernel per step makes the bf16 working copies of all 3x3 filters (not a module, parameter or buffer: no state)
        self._filter_bank = ConvFilterBank([m for m in self.modules() if isinstance(m, (Conv3x3, Conv1x1))])
        # load_state_dict copies into the parameters under no_grad: the cached bf16 / folded filters must not survive it
        self.register_load_state_dict_post_hook(lambda module, incompatible: invalidate_conv_caches())

    def forward(self, x):
        if self.training and torch.is_grad_enabled():
            self._filter_bank.mark_stale()                     # training: the bank is rebuilt every forward, unconditionally
        if torch.is_grad_enabled():
            new_backward_generation(x.device)                  # weight-gradient buffers: one allocation + one fill per pass (any
                                                               # differentiable forward, eval-mode fine-tuning / saliency included)
        x = self.stem(x)
        x = F.dropout(x, p=self.p_dropout, training=self.training)
        return self.stages(x)


def _init_gru(rnn):
    """reference init (model_utils.py:156-184): per-gate uniform(+-sqrt(3/fan_in)) for W_ih and the r,z blocks of W_hh,
    orthogonal for the n block of W_hh, zero biases."""
    def uni(t):
        b = math.sqrt(3.0 / t.shape[1])
        nn.init.uniform_(t, -b, b)

    for name, p in rnn.named_parameters():
        if 'bias' in name:
            nn.init.zeros_(p)
            continue
        h = p.shape[0] // 3
        with torch.no_grad():
            for g in range(3):
                blk = p[g * h:(g + 1) * h]
                if 'weight_hh' in name and g == 2:
                    nn.init.orthogonal_(blk)
                else:
                    uni(blk)


def _init_rnn_reference(rnn):
    """the reference's init_gru (model_utils.py:159-184) restated for the gru / lstm / bilstm decoders, as it behaves: for every
    layer's FORWARD-direction parameters only (``_l{i}``), W_ih and W_hh are split into three row blocks of rows // 3 (for an LSTM
    341 of 1024 rows: the last row keeps torch's default), uniform(+-sqrt(3/fan_in)) per block but orthogonal for the third block of
    W_hh, and both biases are zeroed; every ``_reverse`` parameter keeps torch's default U(+-1/sqrt(H)), biases included."""
    def uni(t):
        b = math.sqrt(3.0 / t.shape[1])
        nn.init.uniform_(t, -b, b)

    with torch.no_grad():
        for i in range(rnn.num_layers):
            for kind, inits in (('weight_ih', (uni, uni, uni)), ('weight_hh', (uni, uni, nn.init.orthogonal_))):
                p = getattr(rnn, '%s_l%d' % (kind, i))
                n = p.shape[0] // 3
                for g, f in enumerate(inits):
                    f(p[g * n:(g + 1) * n])
            nn.init.zeros_(getattr(rnn, 'bias_ih_l%d' % i))
            nn.init.zeros_(getattr(rnn, 'bias_hh_l%d' % i))


class Head(nn.Module):
    def __init__(self, d, n_out):
        super().__init__()
        self.fc1, self.fc2 = _xavier(nn.Linear(d, d // 2)), _xavier(nn.Linear(d // 2, n_out))
        self.drop1, self.drop2 = nn.Dropout(0.2), nn.Dropout(0.2)

    def forward(self, x):
        return self.fc2(self.drop2(F.relu(self.fc1(self.drop1(x)), inplace=True)))


class AttnBlock(nn.Module):
    """one self-attention block after the recurrent stack: y = norm(x + drop(mha(x, x, x)[0])) -- no mask,
    no positional term, no dropout on the probabilities.  Plain torch modules hold the parameters; on the GPU the forward runs
    through attention.attn_block_forward (the HIP attention core and fused add + LayerNorm)."""

    def __init__(self, d, n_heads=8, dropout=0.05):
        super().__init__()
        if n_heads < 1 or d % n_heads != 0:
            raise ValueError('the attention width %d is not divisible into %d heads' % (d, n_heads))
        self.mha = nn.MultiheadAttention(d, n_heads, dropout=0.0, batch_first=True)
        self.norm = nn.LayerNorm(d)
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        if x.is_cuda:
            from .attention import attn_block_forward
            return attn_block_forward(self, x, self.training)
        return self.norm(x + self.drop(self.mha(x, x, x)[0]))


class ConformerBlock(nn.Module):
    """one Conformer block after the recurrent stack, x (B, T, d) float32:
        x1 = x  + 1/2 drop(FF1(norm_ff1(x)))        FF(n) = w2(drop(swish(w1(n))))
        x2 = x1 +     drop(MHSA(norm_att(x1)))      no mask, no positional term, no dropout on the probabilities
        x3 = x2 +     drop(CONV(norm_conv(x2)))     CONV(n) = conv_p2(swish(conv_norm(conv_dw(glu(conv_p1(n))))))
        x4 = x3 + 1/2 drop(FF2(norm_ff2(x3)))
        y  = norm_out(x4)
    conv_dw is a depthwise convolution along time with zero padding, conv_norm a LayerNorm over the channels (a sample stays
    independent of its batch).  Plain torch modules hold the parameters; on the GPU the forward runs through
    conformer.block_forward (the HIP residual / LayerNorm, feed-forward epilogue and convolution-module kernels)."""

    def __init__(self, d, n_heads=8, ff=1024, kernel=7, dropout=0.1):
        super().__init__()
        if n_heads < 1 or d % n_heads != 0:
            raise ValueError('conformer_heads: the width %d is not divisible into %r heads' % (d, n_heads))
        if kernel % 2 != 1 or not 3 <= kernel <= 31:
            raise ValueError('conformer_kernel must be odd and in 3 .. 31, got %r' % (kernel,))
        if ff < 1:
            raise ValueError('conformer_ff must be >= 1, got %r' % (ff,))
        self.norm_ff1, self.ff1_w1, self.ff1_w2 = nn.LayerNorm(d), nn.Linear(d, ff), nn.Linear(ff, d)
        self.norm_att = nn.LayerNorm(d)
        self.mha = nn.MultiheadAttention(d, n_heads, dropout=0.0, batch_first=True)
        self.norm_conv, self.conv_p1 = nn.LayerNorm(d), nn.Linear(d, 2 * d)
        self.conv_dw = nn.Conv1d(d, d, kernel, padding=kernel // 2, groups=d, bias=True)
        self.conv_norm, self.conv_p2 = nn.LayerNorm(d), nn.Linear(d, d)
        self.norm_ff2, self.ff2_w1, self.ff2_w2 = nn.LayerNorm(d), nn.Linear(d, ff), nn.Linear(ff, d)
        self.norm_out = nn.LayerNorm(d)
        self.drop = nn.Dropout(dropout)

    def _ff(self, n, w1, w2):
        return w2(self.drop(F.silu(w1(n))))

    def _conv(self, n):
        v = self.conv_dw(F.glu(self.conv_p1(n), dim=-1).transpose(1, 2)).transpose(1, 2)
        return self.conv_p2(F.silu(self.conv_norm(v)))

    def forward_torch(self, x):
        x = x + 0.5 * self.drop(self._ff(self.norm_ff1(x), self.ff1_w1, self.ff1_w2))
        n = self.norm_att(x)
        x = x + self.drop(self.mha(n, n, n, need_weights=False)[0])
        x = x + self.drop(self._conv(self.norm_conv(x)))
        x = x + 0.5 * self.drop(self._ff(self.norm_ff2(x), self.ff2_w1, self.ff2_w2))
        return self.norm_out(x)

    def forward(self, x):
        if x.is_cuda:
            from .conformer import block_forward
            return block_forward(self, x, self.training)
        return self.forward_torch(x)


DECODER_TYPES = ('gru', 'bigru', 'lstm', 'bilstm')
FREQ_POOLS = ('avg', 'max', 'avg_max')


class Decoder(nn.Module):
    """frequency pool -> 2-layer recurrent decoder (size 256) with dropout 0.3 -> SED head + x/y/z heads (decoders.py:13-154).
    decoder_type 'bigru' (the default), 'gru', 'lstm' or 'bilstm'; freq_pool 'avg' (the default), 'max' or 'avg_max'.  The module
    attribute is ``gru`` or ``lstm``, as in the reference's state dict.  n_attn_layers > 0 (beyond the reference) appends that many
    AttnBlocks of n_attn_heads heads between the recurrent stack and the heads; 0 adds no module and no state-dict key.
    n_conformer_layers > 0 appends that many ConformerBlocks (conformer_heads, conformer_ff, conformer_kernel, conformer_dropout) in
    the same place instead: the two stages exclude each other."""

    def __init__(self, n_in=512, n_classes=12, size=256, decoder_type='bigru', freq_pool='avg', n_attn_layers=0, n_attn_heads=8,
                 attn_dropout=0.05, n_conformer_layers=0, conformer_heads=8, conformer_ff=1024, conformer_kernel=7, conformer_dropout=0.1):
        super().__init__()
        if decoder_type == 'transformer':
            raise NotImplementedError("decoder_type 'transformer' is not implemented (supported: %s)" % ', '.join(DECODER_TYPES))
        if decoder_type not in DECODER_TYPES:
            raise ValueError('invalid decoder_type %r (supported: %s)' % (decoder_type, ', '.join(DECODER_TYPES)))
        if freq_pool not in FREQ_POOLS:
            raise NotImplementedError('freq pooling %r is not implemented (supported: %s)' % (freq_pool, ', '.join(FREQ_POOLS)))
        if n_attn_layers < 0:
            raise ValueError('n_attn_layers must be >= 0, got %r' % (n_attn_layers,))
        if n_conformer_layers < 0:
            raise ValueError('n_conformer_layers must be >= 0, got %r' % (n_conformer_layers,))
        if n_attn_layers > 0 and n_conformer_layers > 0:
            raise ValueError('n_attn_layers and n_conformer_layers exclude each other, got %r and %r' % (n_attn_layers, n_conformer_layers))
        self.n_classes, self.decoder_type, self.freq_pool = n_classes, decoder_type, freq_pool
        bidirectional = decoder_type.startswith('bi')
        if decoder_type == 'bigru':
            self.gru = nn.GRU(n_in, size, num_layers=2, batch_first=True, bidirectional=True, dropout=0.3)
            _init_gru(self.gru)
        elif decoder_type == 'gru':
            self.gru = nn.GRU(n_in, size, num_layers=2, batch_first=True, bidirectional=False, dropout=0.3)
            _init_rnn_reference(self.gru)
        else:
            self.lstm = nn.LSTM(n_in, size, num_layers=2, batch_first=True, bidirectional=bidirectional, dropout=0.3)
            _init_rnn_reference(self.lstm)
        d = (2 if bidirectional else 1) * size
        self.attn = nn.ModuleList(AttnBlock(d, n_attn_heads, attn_dropout) for _ in range(n_attn_layers))
        self.conformer = nn.ModuleList(ConformerBlock(d, conformer_heads, conformer_ff, conformer_kernel, conformer_dropout)
                                       for _ in range(n_conformer_layers))
        self.event = Head(d, n_classes)
        self.x, self.y, self.z = Head(d, n_classes), Head(d, n_classes), Head(d, n_classes)

    @property
    def rnn(self):
        return self.lstm if self.decoder_type in ('lstm', 'bilstm') else self.gru

    def forward(self, feat):
        if self.freq_pool == 'avg':
            seq = freq_mean_sequence(feat)                      # (B, T', 512): mean over frequency
        else:
            seq = freq_pool_sequence(feat, self.freq_pool)      # max / mean + max over frequency
        if seq.is_cuda and GRU_FP32:
            # 0.4 % of the FLOPs but, under bf16 autocast, ~6000 per-timestep cell kernels per forward (torch's native
            # fallback); in float32 the whole sequence goes through MIOpen's fused RNN
            amp = torch.is_autocast_enabled('cuda')
            with torch.autocast(device_type='cuda', enabled=False):
                if self.decoder_type == 'bigru':
                    if FUSED_GRU:
                        from .fused_gru import bigru_forward
                        seq = bigru_forward(self.gru, seq.float(), self.training, half_weights=amp)   # one HIP launch per layer
                    else:
                        seq, _ = self.gru(seq.float())
                else:
                    from .fused_lstm import FUSED_LSTM, rnn_forward
                    if FUSED_LSTM if self.decoder_type in ('lstm', 'bilstm') else FUSED_GRU:
                        seq = rnn_forward(self.rnn, seq.float(), self.training, half_weights=amp)   # one HIP launch per layer
                    else:
                        seq, _ = self.rnn(seq.float())
                for block in self.attn:                         # (float32, like the scans: softmax and LayerNorm statistics)
                    seq = block(seq)
                for block in self.conformer:
                    seq = block(seq)
            # the heads too (0.02 % of the FLOPs): under autocast their eight small linears cost 32 cast kernels per step
            # (weights and biases to bf16, their gradients back) around GEMMs of a few microseconds
            with torch.autocast(device_type='cuda', enabled=False):
                return self._heads(seq.float())
        else:
            seq, _ = self.rnn(seq)
            for block in self.attn:
                seq = block(seq)
            for block in self.conformer:
                seq = block(seq)
        return self._heads(seq)

    def _heads(self, seq):
        if BATCHED_HEADS and seq.dim() == 3:
            return self._heads_batched(seq)
        doa = torch.cat([torch.tanh(self.x(seq)), torch.tanh(self.y(seq)), torch.tanh(self.z(seq))], dim=-1)
        return {'event_frame_logit': self.event(seq), 'doa_frame_output': doa}

    def _heads_batched(self, seq):
        """The four heads (same shapes, same input, independent dropout masks) as ONE batch of four: two batched GEMMs, two
        dropout launches and one tanh instead of eight small GEMMs, eight dropouts, three tanh and a concatenation -- with their
        backward kernels the heads were ~0.45 ms of the 12-ms training step for 0.02 % of its FLOPs.  The parameters stay where
        the reference's state dict has them (event / x / y / z . fc1 / fc2); they are stacked per call (four small copies)."""
        heads = (self.event, self.x, self.y, self.z)
        B, T, D = seq.shape
        w1, b1, w2, b2 = stack_groups([[h.fc1.weight for h in heads], [h.fc1.bias for h in heads],      # (4, D/2, D), (4, D/2),
                                       [h.fc2.weight for h in heads], [h.fc2.bias for h in heads]])     # (4, n_classes, D/2), ...
        b1, b2 = b1.unsqueeze(1), b2.unsqueeze(1)
        x = seq.reshape(1, B * T, D).expand(4, B * T, D)
        x = F.dropout(x, 0.2, self.training)                                # four independent masks (drop1 of each head)
        h = F.relu(torch.baddbmm(b1, x, w1.transpose(1, 2)), inplace=True)
        h = F.dropout(h, 0.2, self.training)
        o = torch.baddbmm(b2, h, w2.transpose(1, 2))                        # (4, B*T, n_classes)
        doa = torch.tanh(o[1:]).permute(1, 0, 2).reshape(B, T, 3 * o.shape[2])   # [x | y | z] along the last axis
        return {'event_frame_logit': o[0].view(B, T, -1), 'doa_frame_output': doa}


_INTERP_IDX = {}


def interpolate_tensor(t, ratio: float):
    """nearest-index resampling along time (model_utils.py:57-75): out[j] = in[floor(j / ratio)]."""
    n_out = int(round(t.shape[1] * float(ratio)))
    r = int(round(float(ratio)))
    if r >= 1 and float(ratio) == r and n_out == r * t.shape[1]:
        # integer ratio (the SELD configuration: 2): floor(j / r) = j // r, i.e. every frame r times -- a broadcast view and one
        # copy, whose backward is one sum, instead of arange / div / floor / index and an index_add into a zero tensor
        return t.unsqueeze(2).expand(t.shape[0], t.shape[1], r, *t.shape[2:]).reshape(t.shape[0], n_out, *t.shape[2:])
    key = (n_out, float(ratio), t.device)
    idx = _INTERP_IDX.get(key)
    if idx is None:
        if len(_INTERP_IDX) > 16:
            _INTERP_IDX.clear()
        idx = _INTERP_IDX[key] = torch.floor(torch.arange(n_out, device=t.device) / float(ratio)).long()
    return t[:, idx]


class SeldCRNN(nn.Module):
    """forward(x (B,7,T,200)) -> dict at the LABEL rate (seld_models.py:39-66: encoder, decoder, then
    interpolate by time_downsample_ratio * label_rate / feature_rate = 16 * 10 / 80 = 2).  decoder_type, freq_pool and
    decoder_size are the reference's YAML keys of the same names (see Decoder); n_attn_layers, n_attn_heads and attn_dropout add
    self-attention blocks after the recurrent decoder (AttnBlock; 0 layers by default: the reference's network); n_conformer_layers,
    conformer_heads, conformer_ff, conformer_kernel and conformer_dropout add Conformer blocks there instead (ConformerBlock; 0 by
    default)."""

    def __init__(self, n_input_channels=7, n_classes=12, label_rate=10, feature_rate=80, decoder_type='bigru', freq_pool='avg',
                 decoder_size=256, n_attn_layers=0, n_attn_heads=8, attn_dropout=0.05, n_conformer_layers=0, conformer_heads=8,
                 conformer_ff=1024, conformer_kernel=7, conformer_dropout=0.1):
        super().__init__()
        self.encoder = Encoder(n_input_channels)
        self.decoder = Decoder(self.encoder.n_output_channels, n_classes, decoder_size, decoder_type, freq_pool,
                               n_attn_layers=n_attn_layers, n_attn_heads=n_attn_heads, attn_dropout=attn_dropout,
                               n_conformer_layers=n_conformer_layers, conformer_heads=conformer_heads, conformer_ff=conformer_ff,
                               conformer_kernel=conformer_kernel, conformer_dropout=conformer_dropout)
        self.ratio = self.encoder.time_downsample_ratio * label_rate / feature_rate

    def forward(self, x):
        out = self.decoder(self.encoder(x))
        return {k: interpolate_tensor(v, self.ratio) for k, v in out.items()}

    def pack_parameters(self):
        """Lay the parameters the decoder stacks every step (the two directions of each GRU parameter, the four heads' weights) out
        stacked in memory, so that the stack is a view instead of a copy (nn_ops.pack_stacked_parameters).  Values, Parameter
        objects and state-dict keys are unchanged.  Call it after the last ``.to(device)`` (the Trainer does); returns self."""
        from .nn_ops import pack_stacked_parameters
        gru, dec = self.decoder.rnn, self.decoder
        directions = ('', '_reverse') if gru.bidirectional else ('',)
        groups = [[getattr(gru, '%s_l%d%s' % (kind, layer, rev)) for rev in directions]
                  for layer in range(gru.num_layers) for kind in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
        heads = (dec.event, dec.x, dec.y, dec.z)
        groups += [[h.fc1.weight for h in heads], [h.fc1.bias for h in heads], [h.fc2.weight for h in heads], [h.fc2.bias for h in heads]]
        pack_stacked_parameters(groups)
        if hasattr(gru, '_flat_weights'):      # nn.GRU / nn.LSTM cache references to their weights for the (unused here) MIOpen path
            gru._flat_weights = [getattr(gru, n) if hasattr(gru, n) else None for n in gru._flat_weights_names]
        return self

    def load_reference_state_dict(self, sd, strict: bool = True):
        """Load weights trained with the reference (``torch.load(ckpt)`` or its ``['state_dict']``, experiments/inference.py:
        115-116): see salsa_amd/crnn/checkpoint.py."""
        from .checkpoint import load_reference_state_dict
        return load_reference_state_dict(self, sd, strict)

    def reference_state_dict(self):
        """This model's state dict under the reference's key names."""
        from .checkpoint import reference_state_dict
        return reference_state_dict(self)
