"""Inference-graph tooling: turning a QAT model into the graph that is deployed -- the MI355X counterpart of the reference's
``wbwtab/bn_fuse/bn_fuse.py:20-107``, ``wqaq/iao/bn_fuse/bn_fuse.py:20-80`` and the pre-quantisation loop of
``wqaq/dorefa/quant_model_test/quant_model_test.py:189-191``.

  * ``prequantize_weights``: ``m.weight.data = m.weight_quantizer(m.weight)`` for every ``quant_inference=True`` layer (the stored weights ARE the
    fake-quantised ones; the forward then skips the weight quantizer);
  * ``wbwtab_model_bn_fuse``: BatchNorm folded into the convolution in front of it.  In front of a BINARY activation the fold needs no multiplier --
    sign(gamma * (y - mean) / std + beta) = sign(+-(y - mean + beta * std / gamma)) -- so the folded weights stay ternary / binary codes x alpha and
    only a bias (and the weights' sign where gamma < 0) changes (ref 36-55); elsewhere the ordinary w * gamma / std fold (ref 56-59);
  * ``iao_model_bn_fuse``: ``QuantBNFuseConv2d`` -> ``QuantConv2d(quant_inference=True)`` with w * gamma / std, beta + (b - mean) * gamma / std and the
    trained quantizer scales / zero points copied over (ref 20-66).
The results are ordinary modules of this package: in eval mode they run on the same gfx950 kernels (activation codes, integer accumulators).
``tests/test_gpu_inference.py`` checks train-graph == inference-graph on the same batch, as the reference's ``*_test.py`` scripts do.

  * ``wbwtab_compile_bits``: the folded W-ternary / W-binary, A-binary graph compiled into a flat plan that keeps ONE BIT per hidden activation
    (``csrc/qgemm_bits.hip``: XNOR / AND / popcount against bit-plane weight tables, bias and alpha folded into an integer threshold per channel).  It computes
    exactly what the folded graph computes -- same signs in every hidden stage, same logits to the bit.  ``bit_ends=True``: the two ends stay on bits as well -- the
    first conv writes activation bits in one launch (``mn_conv2d_first_sign_bits``), the classifier reads them (``mn_bitsconv1x1_small_fwd``).

  * ``dorefa_compile_codes``: a pre-quantised DoReFa W2A2 ``quant_inference=True`` net compiled into a flat plan that keeps TWO BITS per hidden activation
    (``csrc/qgemm_codes.h``: activation codes as bit planes, plane-serial popcounts against weight code planes, the block's BatchNorm + ReLU + quantizer as integer
    thresholds per channel).  One kernel per hidden block, packed codes in, packed codes out; same codes in every hidden stage as the eval-mode model.
    ``tile_blocks=True`` adds plain ``nin``: its dense 5x5 block on an LDS tile and its 3x3 / stride 2 max-pools on the planes.

  * ``iao_compile_int8``: the BN-folded, pre-quantised symmetric IAO graph compiled into a flat plan that keeps ONE INT8 CODE per hidden activation
    (``csrc/qgemm_iao8.h``: byte codes against weight-code bytes on v_mfma_i32_16x16x64_i8, bias + ReLU + [2x2 max-pool] + the consumer's quantizer in the epilogue).
    One kernel per hidden block; the two ends stay on the model's own modules.  A BN-folded IAO ResNet compiles by the same call (``csrc/qgemm_iao8_res.h``: strided
    convs, shortcut convs and the QuantAdd on byte codes, one code map per consumer quantizer of a block's output).  ``zero_points=True`` admits asymmetric
    quantizers on the sequential nets (``csrc/qgemm_iao8_zp.h``: the zero points as integer offsets of the exact int32 sum)."""
import copy
import ctypes as C

import torch
import torch.nn as nn


def mark_stored_codes(m):
    """Record that the weights m.weight holds RIGHT NOW are codes x alpha[o] (wbwtab QuantConv2d with quant_inference=True): the verdict is tied to the tensor's data
    pointer and version, so `weight.data = ...`, an in-place update or load_state_dict (pre-hook) drop it; Module._apply (.cuda(), .to()) carries it over."""
    m.stored_codes = True
    m._mn_codes_key = (m.weight.data_ptr(), m.weight._version)


@torch.no_grad()
def prequantize_weights(model):
    """For every layer built with ``quant_inference=True``: store the fake-quantised weights (what ``quant_model_test.py:189-191`` does after loading)."""
    n = 0
    for m in model.modules():
        if getattr(m, "quant_inference", False) and hasattr(m, "weight_quantizer") and hasattr(m, "weight"):
            was = m.weight_quantizer.training
            m.weight_quantizer.eval()                  # IAO: do not move the trained observer / scale
            m.weight.data = m.weight_quantizer(m.weight).detach()
            m.weight_quantizer.train(was)
            n += 1
            if type(m).__module__.endswith("wbwtab.quantize") and hasattr(m, "stored_codes") and getattr(m.weight_quantizer, "W", 0) in (2, 3):
                mark_stored_codes(m)           # the stored weights ARE the quantizer's output t * alpha[o]: the layer keeps contracting integer codes
            # DoReFa layers: record the "stored weights lie on the quantizer grid" verdict now (one host sync per layer, here instead of inside the first forward --
            # which may be a captured one)
            if type(m).__module__.endswith("dorefa.quantize") and m.weight.is_cuda and not torch.cuda.is_current_stream_capturing():
                from micronet_amd.quantization.wqaq.dorefa.quantize import _weight_is_coded
                m.__dict__.pop("_mn_grid", None)
                _weight_is_coded(m)
    return n


def _conv_like(conv, cls, **kw):
    return cls(conv.in_channels, conv.out_channels, conv.kernel_size, stride=conv.stride, padding=conv.padding, dilation=conv.dilation,
               groups=conv.groups, bias=True, padding_mode=conv.padding_mode, **kw)


@torch.no_grad()
def wbwtab_model_bn_fuse(model, W=2, inplace=False):
    """ref wbwtab/bn_fuse/bn_fuse.py:20-107.  ``model``: prepared with ``quant_inference=True`` and its weights pre-quantised or not (the fold acts on
    whatever ``conv.weight`` holds, as the reference does).  BN layers are counted in module order; the first ``bin_bn_fuse_num`` of them (= the
    number of binary ``ActivationQuantizer``s) sit in front of a binary activation."""
    from micronet_amd.quantization.wbwtab import quantize
    if not inplace:
        model = copy.deepcopy(model)
    bin_bn_fuse_num = sum(isinstance(m, quantize.ActivationQuantizer) for m in model.modules())
    counter = [0]

    def fuse(conv, bn):
        counter[0] += 1
        k = counter[0]
        mean, std, gamma, beta = bn.running_mean, torch.sqrt(bn.running_var + bn.eps), bn.weight, bn.bias
        w = conv.weight
        b = conv.bias if conv.bias is not None else mean.new_zeros(mean.shape)
        if 1 <= k <= bin_bn_fuse_num:
            w_f, b_f = w.clone(), b.clone()
            pos, neg = gamma.gt(0), gamma.lt(0)
            b_f[pos] = b[pos] - mean[pos] + beta[pos] * (std[pos] / gamma[pos])
            w_f[neg] = w[neg] * -1
            b_f[neg] = mean[neg] - b[neg] - beta[neg] * (std[neg] / gamma[neg])
        else:
            w_f = w * (gamma / std).reshape([conv.out_channels, 1, 1, 1])
            b_f = beta + (b - mean) * (gamma / std)
        if 2 <= k <= bin_bn_fuse_num:
            new = _conv_like(conv, quantize.QuantConv2d, W=W, quant_inference=True)
            new.in_shuffle_groups = getattr(conv, "in_shuffle_groups", 0)
            # The low-bit deployed path: in front of a binary activation the fold leaves the weights codes x alpha[o] (only signs and the bias change, ref 36-55).
            # Checked here, once: every non-zero |w| of an output channel equals the channel's maximum -- then the layer contracts the +-1 input codes against
            # integer weight codes on the matrix cores and (where prepare() had established conv -> bn -> sign in this order: ``lazy_for_bn``) hands its
            # un-computed result to the sign behind it, exactly like the training graph in eval mode: one byte per activation end to end.
            mag = w_f.detach().abs().flatten(1)
            coded = bool(((mag == 0) | (mag == mag.amax(1, keepdim=True))).all()) and W in (2, 3)
            new.lazy_for_bn = bool(coded and getattr(conv, "lazy_for_bn", False))
        else:
            new = _conv_like(conv, nn.Conv2d)
            from micronet_amd.nn import Conv2dFirst, Conv2dSignIn
            if type(conv) in (Conv2dFirst, Conv2dSignIn):
                new.__class__ = type(conv)          # the fp32 first / last conv keep their gfx950 kernels (same parameters: only the forward differs)
        new = new.to(w.device)
        new.weight.data, new.bias.data = w_f, b_f
        if 2 <= k <= bin_bn_fuse_num and coded:
            mark_stored_codes(new)
        return new

    def walk(module):
        last, packed_bn = None, False
        for name, child in module.named_children():
            if isinstance(child, nn.Conv2d):
                last = (name, child)
            elif isinstance(child, nn.BatchNorm2d):
                module._modules[last[0]] = fuse(last[1], child)
                module._modules[name] = nn.Identity()
                packed_bn = isinstance(child, quantize.BatchNorm2dBinAct) and bool(child.packed)      # (prepare() established bn -> sign adjacency for this block)
            elif isinstance(child, quantize.ActivationQuantizer):
                if packed_bn and child.A == 2:
                    child.deploy_packed = True      # conv -> Identity -> sign on the packed kernels (ActivationQuantizer.forward)
                packed_bn = False
            else:
                packed_bn = False
                walk(child)
    walk(model)
    return model


@torch.no_grad()
def iao_model_bn_fuse(model, inplace=False):
    """ref wqaq/iao/bn_fuse/bn_fuse.py:20-80: every ``QuantBNFuseConv2d`` becomes a ``QuantConv2d(quant_inference=True)`` holding the folded (not yet
    quantised) weights and the trained quantizer state; follow with ``prequantize_weights``."""
    from micronet_amd.quantization.wqaq.iao import quantize
    if not inplace:
        model = copy.deepcopy(model)

    def fuse(m):
        mean, std = m.running_mean, torch.sqrt(m.running_var + m.eps)
        b = m.bias if m.bias is not None else mean.new_zeros(mean.shape)
        aq, wq = m.activation_quantizer, m.weight_quantizer
        q_level = 0 if getattr(wq.observer, "q_level", "L") != "L" else 1          # per-channel iff the weight observer is (an out_channels == 1 conv has ONE scale either way)
        new = _conv_like(m, quantize.QuantConv2d, a_bits=aq.bits, w_bits=wq.bits, q_type=wq._q_type_static, q_level=q_level, quant_inference=True).to(m.weight.device)
        new.weight.data = m.weight * (m.gamma / std).reshape([m.out_channels, 1, 1, 1])
        new.bias.data = m.beta + (b - mean) * (m.gamma / std)
        for src, dst in ((aq, new.activation_quantizer), (wq, new.weight_quantizer)):
            dst.scale.copy_(src.scale)
            dst.zero_point.copy_(src.zero_point)
            dst.eps = src.eps
            dst.q_type = src.q_type
            dst.observer.min_val.copy_(src.observer.min_val)
            dst.observer.max_val.copy_(src.observer.max_val)
            dst.observer.num_flag = 1
        return new

    def walk(module):
        for name, child in module.named_children():
            if isinstance(child, quantize.QuantBNFuseConv2d):
                module._modules[name] = fuse(child)
                if getattr(child, "in_shuffle_groups", 0) > 1 and getattr(module, "shuffle_groups", 0) == child.in_shuffle_groups and hasattr(module, "channel_shuffle_flag"):
                    module.channel_shuffle_flag = 1          # prepare(fuse_blocks=True) had folded the block's shuffle into the BN-fused conv: hand it back to the block
            else:
                walk(child)
    walk(model)
    return model


# ------------------------------------------------------------------------------------------------ bit-packed deployment (csrc/qgemm_bits.hip)
def _err(msg):
    from micronet_amd._lib import MicronetHipError
    return MicronetHipError(msg)


def _net_sequence(model, who):
    """(seq, prefix, flatten) of a model that is an nn.Sequential of blocks, or the reference's Net holding one (models/nin_gc.py:144-147: forward = model(x).view(N, -1))."""
    if isinstance(model, nn.Sequential):
        return model, "", False
    kids = list(model.named_children())
    if len(kids) != 1 or not isinstance(kids[0][1], nn.Sequential):
        raise _err("%s: module order not recognised (%s: expected an nn.Sequential of blocks, or the reference's Net holding one)" % (who, type(model).__name__))
    return kids[0][1], kids[0][0] + ".", True


def _shuffle_in_front(who, nm, child, conv):
    """The groups of the channel shuffle in front of ``conv`` -- its own ``in_shuffle_groups`` or its block's -- or 0."""
    s = int(getattr(conv, "in_shuffle_groups", 0) or 0)
    if getattr(child, "channel_shuffle_flag", 0) and getattr(child, "shuffle_groups", 1) > 1:
        if s > 1:
            raise _err("%s: %s: two channel shuffles in front of one conv" % (who, nm))
        s = int(child.shuffle_groups)
    return s if s > 1 else 0


def _check_shuffle_divides(who, nm, conv, s):
    if conv.in_channels % s:
        raise _err("%s: %s: %d input channels cannot be shuffled in %d groups" % (who, nm, conv.in_channels, s))


def _shuffle_order(C_, s, device):
    """position j of a consumer's shuffled input is its producer's channel (j % s) * (C / s) + j // s (models/nin_gc.py:4-15)"""
    j = torch.arange(C_, device=device)
    return ((j % s) * (C_ // s) + j // s).to(torch.int32).contiguous()


def _require_gpu(model, who):
    for p_ in model.parameters():
        if not p_.is_cuda:
            raise _err("%s: the model is on %s: micronet_amd runs on MI355X only (no CPU fallback)" % (who, p_.device))


def _one(v):
    """The value of a pair that is the same in both directions, else -1."""
    return v[0] if v[0] == v[1] else -1


def _out_size(v, k, s, p, d):
    """The output extent of a conv along one direction."""
    return (v + 2 * p - d * (k - 1) - 1) // s + 1


def _conv_geom(conv, N=1, H=4, W=4, in_shuffle=0):
    """The ConvGeom of a conv module's own fields on an N x H x W input; the shape-independent calls take the default."""
    from micronet_amd import _lib
    return _lib.ConvGeom(N, conv.in_channels, H, W, conv.out_channels, conv.kernel_size[0], conv.kernel_size[1], conv.stride[0], conv.stride[1], conv.padding[0],
                         conv.padding[1], conv.dilation[0], conv.dilation[1], conv.groups, in_shuffle)


def _block_geom(L, N=1, H=4, W=4):
    """The ConvGeom of a layer's dict (square kernel; stride 1 and one group where the dict names neither) on an N x H x W input; the shape-independent calls take
    the default."""
    from micronet_amd import _lib
    s = L.get("stride", 1)
    return _lib.ConvGeom(N, L["cin"], H, W, L["cout"], L["k"], L["k"], s, s, L["pad"], L["pad"], 1, 1, L.get("groups", 1), 0)


class _Plan(nn.Module):
    """What the three compiled plans share: the model's own two ends and tail, the layer dicts, eval only, one set of buffers per first-block output shape."""
    who = None          # the entry point's name in the plan's messages

    def __init__(self, first, layers, last, tail, flatten, report):
        super().__init__()
        self.first, self.last, self.tail = first, last, nn.ModuleList(tail)
        self.layers, self.flatten, self.report = layers, flatten, report
        self.keep_stages = False          # True: forward also leaves every stage's buffer in ``stage_bits`` / ``stage_codes`` (tests)
        self._ws = {}
        self.eval()

    def train(self, mode=True):
        if mode:
            raise _err("%s: the compiled plan is eval-only" % self.who)
        return super().train(False)

    def _shape_buffers(self, shape, device):
        """What ``_plan_buffers`` makes for one first-block output shape: allocated once, reused by every later call."""
        key = (tuple(shape), str(device))
        if key not in self._ws:
            self._ws[key] = self._plan_buffers(shape, device)
        return self._ws[key]

    @staticmethod
    def _after_conv(block, conv, y):
        kids = list(block.children())
        for m in kids[kids.index(conv) + 1:]:          # what follows the conv inside the block
            y = m(y)
        return y

    def _finish(self, y):
        for m in self.tail:
            y = m(y)
        return y.view(y.size(0), -1) if self.flatten else y


def _codes_of(t):
    from micronet_amd.sign_tensor import SignTensor
    c = t.codes if isinstance(t, SignTensor) else t
    if not (torch.is_tensor(c) and c.is_cuda and c.dtype == torch.int8 and c.dim() == 4):
        raise _err("pack_bits: needs a SignTensor or an int8 +-1 tensor [N, C, H, W] on the GPU (no CPU fallback)")
    return c.contiguous()


def pack_bits(t):
    """int8 +-1 codes [N, C, H, W] (or a SignTensor) -> int32 tensor [N, ceil(C / 32), H, W] of uint32 words: bit c & 31 of word c >> 5 is 1 iff the activation is +1."""
    from micronet_amd import ops
    c = _codes_of(t)
    N, Cc, H, W = c.shape
    bits = torch.empty((N, (Cc + 31) // 32, H, W), dtype=torch.int32, device=c.device)
    ops._call("mn_bits_pack_sign8", ops._p(c), N, Cc, H * W, ops._p(bits), ops._s())
    return bits


def unpack_bits(bits, C):
    """The inverse of ``pack_bits``: int8 +-1 codes [N, C, H, W]."""
    from micronet_amd import ops
    if not (torch.is_tensor(bits) and bits.is_cuda and bits.dtype == torch.int32 and bits.dim() == 4 and bits.shape[1] == (int(C) + 31) // 32):
        raise _err("unpack_bits: needs an int32 word tensor [N, ceil(C / 32), H, W] on the GPU")
    bits = bits.contiguous()
    N, _, H, W = bits.shape
    out = torch.empty((N, int(C), H, W), dtype=torch.int8, device=bits.device)
    ops._call("mn_bits_unpack_sign8", ops._p(bits), N, int(C), H * W, ops._p(out), ops._s())
    return out


def _pool_kind(m):
    """(kernel, stride, padding) of a max-pool the bit kernels cover -- 2x2 / 2 / 0 (models/nin_gc.py) and 3x3 / 2 / 1 (models/nin.py), floor mode -- else None."""
    if not isinstance(m, nn.MaxPool2d) or m.ceil_mode or m.return_indices or m.dilation not in (1, (1, 1), [1, 1]):
        return None
    one = lambda v: v if isinstance(v, int) else (v[0] if len(v) == 2 and v[0] == v[1] else None)
    ksp = (one(m.kernel_size), one(m.stride if m.stride is not None else m.kernel_size), one(m.padding))
    return ksp if ksp in ((2, 2, 0), (3, 2, 1)) else None


def _bitconv_mfma_kernel_name(fold):
    """The kernel mn_bitconv_mfma_fwd reports for a 1x1 hidden block (csrc/qgemm_bits_mfma.h); fold: 0 or 1."""
    return "k_bitconv_mfma<%d>" % fold


def _bitconv_mfma3_kernel_name():
    """The kernel mn_bitconv_mfma3_fwd reports for a 3x3 hidden block (csrc/qgemm_bits_mfma3.h)."""
    return "k_bitconv_mfma3<0>"


def _conv_kernel_name(k, cin, groups, fold):
    """The kernel mn_bitconv_fwd launches for a hidden block (csrc/qgemm_bits.hip: the dispatch at the end of the file); fold: 0, 1 (2x2 / 2) or 2 (3x3 / 2 / 1)."""
    cw, cg = (cin + 31) // 32, cin // groups
    if k == 5:
        return "k_bitconv_tile<5,%d>" % (3 if cw == 3 else 0)
    if fold == 2:
        return "k_bitconv1_pool3<%d>" % (8 if groups == 1 and cw <= 8 else 0)
    nw = max(((gi * cg + cg - 1) >> 5) - ((gi * cg) >> 5) + 1 for gi in range(groups))
    sel = nw if (nw == 1 or (k == 1 and nw in (2, 4))) else 0
    return "k_bitconv<%d,%d,%d>" % (k, sel, fold)


class BitPlan(_Plan):
    """What ``wbwtab_compile_bits`` returns: first block (fp32 conv + sign, the folded graph's own module) -> bit pack -> n XNOR-popcount blocks (max-pools folded in,
    or run on the bits behind a block that cannot fold them) -> bit unpack -> last block and tail (the folded graph's own modules).  Eval only; owns the packed weight
    tables and one set of bit buffers per input shape.  ``bit_ends``: the first conv's kernel writes the first stage's bits itself (no fp32 map, no int8 codes, no
    pack) and the last conv reads the last stage's bits (no unpack, no int8 buffer); what follows the last conv inside its block, and the tail, run unchanged."""

    who = "wbwtab_compile_bits"

    def __init__(self, first, layers, last, tail, flatten, report, bit_ends=False):
        super().__init__(first, layers, last, tail, flatten, report)          # layers: dicts of geometry, table, pool, out_order
        self.bit_ends = bool(bit_ends)
        self.stage_bits = []

    def _plan_buffers(self, shape, device):
        """Bit buffers (and the int8 buffer in front of the last conv) for one first-block output shape."""
        from micronet_amd import _lib
        N, Cc, H, W = shape
        g0 = None
        if self.bit_ends:
            conv = self.first.conv
            g0 = _conv_geom(conv, N, H, W)          # (Cc is conv.out_channels: forward hands over the first conv's own output shape)
            if not _lib.get_lib().mn_conv2d_first_sign_bits_supported(C.byref(g0)):
                raise _err("wbwtab_compile_bits(bit_ends=True): %s.conv: a %d x %d x %d x %d input is not covered by mn_conv2d_first_sign_bits (W %% 4 == 0, H * W %% 32 == 0, "
                           "the image strip in LDS)" % (self.report[0]["name"], N, conv.in_channels, H, W))
        bufs, geoms = [torch.empty((N, (Cc + 31) // 32, H, W), dtype=torch.int32, device=device)], []
        mids = []
        for L in self.layers:
            k, p = L["k"], L["pad"]
            geoms.append(_block_geom(L, N, H, W))
            H, W = H + 2 * p - k + 1, W + 2 * p - k + 1
            pool = L["pool_ksp"]
            if pool and (min(H, W) + 2 * pool[2] < pool[0] or (L["pool"] == 1 and (H % 2 or W % 2))):
                raise _err("wbwtab_compile_bits: %s: the max-pool behind it does not fit a %d x %d map" % (L["name"], H, W))
            mids.append(torch.empty((N, (L["cout"] + 31) // 32, H, W), dtype=torch.int32, device=device) if pool and not L["pool"] else None)
            if pool:
                H, W = (H + 2 * pool[2] - pool[0]) // pool[1] + 1, (W + 2 * pool[2] - pool[0]) // pool[1] + 1
            bufs.append(torch.empty((N, (L["cout"] + 31) // 32, H, W), dtype=torch.int32, device=device))
            Cc = L["cout"]
        if self.bit_ends:
            if not _lib.get_lib().mn_bitsconv1x1_small_supported(Cc, H * W, self.last.conv.out_channels):
                raise _err("wbwtab_compile_bits(bit_ends=True): %s.conv: a %d-channel %d x %d map is not covered by mn_bitsconv1x1_small_fwd (its lanes own 4 consecutive "
                           "pixels: H * W %% 4 == 0; the weights in LDS)" % (self.report[-1]["name"], Cc, H, W))
            return (bufs, geoms, None, mids, g0)
        if (H * W) % 4:
            raise _err("wbwtab_compile_bits: %s: its %d x %d output cannot be unpacked for the last conv (mn_bits_unpack_sign8 needs H * W %% 4 == 0)"
                       % (self.layers[-1]["name"], H, W))
        return (bufs, geoms, torch.empty((N, Cc, H, W), dtype=torch.int8, device=device), mids, g0)

    @torch.no_grad()
    def forward(self, x):
        from micronet_amd import ops
        from micronet_amd.sign_tensor import SignTensor
        if self.bit_ends:
            conv = self.first.conv
            if not (type(x) is torch.Tensor and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == conv.in_channels):
                raise _err("wbwtab_compile_bits(bit_ends=True): the input must be a float32 GPU tensor [N, %d, H, W] (no CPU fallback)" % conv.in_channels)
            x = x.contiguous()
            bufs, geoms, a8, mids, g0 = self._shape_buffers((x.shape[0], conv.out_channels, x.shape[2], x.shape[3]), x.device)
            st = ops._s()
            ops._call("mn_conv2d_first_sign_bits", C.byref(g0), ops._p(x), ops._p(ops._chk(conv.weight.detach(), "weight")), ops._p(ops._chk(conv.bias, "bias")),
                      ops._p(bufs[0]), st)
        else:
            a = self.first(x)
            if not isinstance(a, SignTensor):
                raise _err("wbwtab_compile_bits: the first block did not produce packed signs (input must be a contiguous float32 GPU tensor with H * W % 4 == 0)")
            codes = a.codes.contiguous()
            N, Cc, H, W = codes.shape
            bufs, geoms, a8, mids, _ = self._shape_buffers(codes.shape, codes.device)
            st = ops._s()
            ops._call("mn_bits_pack_sign8", ops._p(codes), N, Cc, H * W, ops._p(bufs[0]), st)
        for i, L in enumerate(self.layers):
            fwd = "mn_bitconv_mfma_fwd" if L.get("mfma") else "mn_bitconv_mfma3_fwd" if L.get("mfma3") else "mn_bitconv_fwd"
            if mids[i] is None:
                ops._call(fwd, C.byref(geoms[i]), ops._p(L["table"]), ops._p(bufs[i]), ops._p(bufs[i + 1]), int(L["pool"]), st)
            else:          # a pool the block cannot fold: the block at full size, then the word-wise OR
                m, (pk, ps, pp) = mids[i], L["pool_ksp"]
                ops._call(fwd, C.byref(geoms[i]), ops._p(L["table"]), ops._p(bufs[i]), ops._p(m), 0, st)
                ops._call("mn_bits_maxpool", ops._p(m), m.shape[0], m.shape[1], m.shape[2], m.shape[3], pk, ps, pp, ops._p(bufs[i + 1]), st)
        if self.keep_stages:
            self.stage_bits = [b.clone() for b in bufs]
        if self.bit_ends:
            conv = self.last.conv
            n_, _, h_, w_ = bufs[-1].shape
            y = torch.empty((n_, conv.out_channels, h_, w_), dtype=torch.float32, device=bufs[-1].device)
            ops._call("mn_bitsconv1x1_small_fwd", ops._p(bufs[-1]), ops._p(ops._chk(conv.weight.detach(), "weight")), ops._p(ops._chk(conv.bias, "bias")), ops._p(y),
                      n_, conv.in_channels, h_ * w_, conv.out_channels, st)
            y = self._after_conv(self.last, conv, y)          # (Identity, ReLU)
        else:
            n_, c_, h_, w_ = a8.shape
            ops._call("mn_bits_unpack_sign8", ops._p(bufs[-1]), n_, c_, h_ * w_, ops._p(a8), st)
            y = self.last(SignTensor(a8))
        return self._finish(y)


def _check_ends(who, first, nm_first, last, nm_last, first_kernel, first_supported, last_kernel, last_supported):
    """Both ends must be covered by their kernels -- never a silent byte path.  Shape-independent part (the input shape is checked by the plan).  ``first_supported(g)``
    / ``last_supported(cin, hw, cout)``: the library's verdicts; ``*_kernel``: the names in the messages."""
    conv = first.conv
    if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
        raise _err("%s: %s.conv: padding mode not covered by %s" % (who, nm_first, first_kernel))
    g = _conv_geom(conv, 1, 8, 8)
    if not first_supported(g):
        raise _err("%s: %s.conv: not covered by %s (%dx%d, stride %d, padding %d, dilation %d, groups %d, %d taps per output: needs \"same\" padding, stride 1, groups 1, "
                   "at most 76 taps)" % (who, nm_first, first_kernel, conv.kernel_size[0], conv.kernel_size[1], conv.stride[0], conv.padding[0], conv.dilation[0], conv.groups,
                                         conv.in_channels // conv.groups * conv.kernel_size[0] * conv.kernel_size[1]))
    conv = last.conv
    one = lambda v, k: tuple(v) == (k, k)
    if not (conv.padding_mode == "zeros" and not isinstance(conv.padding, str) and one(conv.kernel_size, 1) and one(conv.stride, 1) and one(conv.padding, 0) and
            one(conv.dilation, 1) and conv.groups == 1 and last_supported(conv.in_channels, 4, conv.out_channels)):
        raise _err("%s: %s.conv: the last conv is not the small 1x1 classifier %s covers (%dx%d, stride %d, padding %s, groups %d, %d -> %d channels: needs 1x1, stride 1, "
                   "no padding, groups 1, at most 16 outputs)"
                   % (who, nm_last, last_kernel, conv.kernel_size[0], conv.kernel_size[1], conv.stride[0], conv.padding, conv.groups, conv.in_channels, conv.out_channels))


def _check_bit_ends(first, nm_first, last, nm_last):
    """``bit_ends=True``: ``_check_ends`` for the two bit kernels, and no channel shuffle in front of the last conv."""
    from micronet_amd import _lib
    lib = _lib.get_lib()
    _check_ends("wbwtab_compile_bits(bit_ends=True)", first, nm_first, last, nm_last, "mn_conv2d_first_sign_bits", lambda g: lib.mn_conv2d_first_sign_bits_supported(C.byref(g)),
                "mn_bitsconv1x1_small_fwd", lib.mn_bitsconv1x1_small_supported)
    if getattr(last, "channel_shuffle_flag", 0) and getattr(last, "shuffle_groups", 1) > 1:
        raise _err("wbwtab_compile_bits(bit_ends=True): %s: a channel shuffle in front of the last conv is not covered by mn_bitsconv1x1_small_fwd" % nm_last)


def _walk_bits(model, bit_ends=False, mfma_blocks=False, mfma_k3=False):
    """The graph walk of ``wbwtab_compile_bits`` (no GPU needed): (first, layers, last, tail, flatten, report).  ``mfma_blocks``: a hidden block
    ``mn_bitconv_mfma_supported`` covers, whose fold is 0 or 1, runs on the MFMA form (``layer["mfma"]``); ``mfma_k3``: a hidden 3x3 block ``mn_bitconv_mfma3_supported``
    covers, with no folded pool, runs on the 3x3 MFMA form (``layer["mfma3"]``).  Neither refuses anything: a block they do not cover keeps its kernel."""
    from micronet_amd import _lib
    from micronet_amd.nn import Conv2dFirst
    from micronet_amd.quantization.wbwtab import quantize
    seq, prefix, flatten = _net_sequence(model, "wbwtab_compile_bits")
    for n_, m in model.named_modules():
        if isinstance(m, quantize.ActivationQuantizer) and m.A != 2:
            raise _err("wbwtab_compile_bits: %s has A = %d; only binary activations (A = 2) are bit-packed" % (n_, m.A))
    first = last = None
    layers, tail, report = [], [], []
    for name, child in seq.named_children():
        nm = prefix + name
        if last is not None:
            tail.append(child)
            continue
        if isinstance(child, nn.MaxPool2d):
            ksp = _pool_kind(child)
            if ksp is None:
                raise _err("wbwtab_compile_bits: %s: max-pool (kernel %s, stride %s, padding %s, ceil_mode %s) is not covered by the bit kernels (2x2 / 2 / 0 and 3x3 / 2 / 1, "
                           "floor mode)" % (nm, child.kernel_size, child.stride, child.padding, child.ceil_mode))
            if not layers or layers[-1]["pool_ksp"]:
                raise _err("wbwtab_compile_bits: %s: a %dx%d max-pool is folded only into the bit block directly in front of it" % (nm, ksp[0], ksp[0]))
            L = layers[-1]
            # folded where the block's kernel can own a pooled pixel (2x2: 1x1 and 3x3 blocks; 3x3 / 2: 1x1 blocks), else mn_bits_maxpool behind the block
            L["pool"] = (1 if L["k"] in (1, 3) else 0) if ksp == (2, 2, 0) else (2 if L["k"] == 1 else 0)
            L["pool_ksp"], L["stage"] = ksp, name
            continue
        conv, bn, act = getattr(child, "conv", None), getattr(child, "bn", None), getattr(child, "relu", None)
        if not (quantize._is_ref_block(child) and isinstance(conv, nn.Conv2d) and isinstance(bn, nn.Identity)):
            raise _err("wbwtab_compile_bits: %s (%s): module order not recognised (expected a BN-folded conv -> Identity -> activation block)" % (nm, type(child).__name__))
        if first is None:
            if not (type(conv) is Conv2dFirst and isinstance(act, quantize.ActivationQuantizer) and act.deploy_packed) or getattr(child, "channel_shuffle_flag", 0):
                raise _err("wbwtab_compile_bits: %s: the first block must be the fp32 first conv followed by a packed binary activation" % nm)
            first = child
            report.append(dict(name=nm, kind="first", K=conv.in_channels // conv.groups * conv.kernel_size[0] * conv.kernel_size[1], words=0,
                               kernel="first conv + mn_bnsign_fwd_i8, k_bits_pack", pooled=False, out_order="identity", stage=name))
            continue
        if not isinstance(conv, quantize.QuantConv2d):
            if not layers:
                raise _err("wbwtab_compile_bits: %s: no quantised block between the first and the last conv" % nm)
            last = child
            report.append(dict(name=nm, kind="last", K=conv.in_channels // conv.groups * conv.kernel_size[0] * conv.kernel_size[1], words=(conv.in_channels + 31) // 32,
                               kernel="k_bits_unpack, last conv on sign codes", pooled=False, out_order="identity", stage=name))
            continue
        # ---- a hidden block: sign(conv(a, t * alpha) + b)
        if not isinstance(act, quantize.ActivationQuantizer):
            raise _err("wbwtab_compile_bits: %s: a quantised conv that is not followed by a binary activation" % nm)
        if not conv._codes_valid():
            raise _err("wbwtab_compile_bits: %s.conv: the stored weights are not codes x alpha (fold the model AFTER prequantize_weights)" % nm)
        if tuple(conv.stride) != (1, 1) or tuple(conv.dilation) != (1, 1) or conv.padding_mode != "zeros" or isinstance(conv.padding, str):
            raise _err("wbwtab_compile_bits: %s.conv: stride / dilation other than 1 (or non-zero padding mode) is not covered by the bit kernels" % nm)
        k, pad = conv.kernel_size[0], conv.padding[0]
        shuffle = _shuffle_in_front("wbwtab_compile_bits", nm, child, conv)
        g = _conv_geom(conv)          # (stride and dilation are 1: anything else was refused above)
        if not _lib.get_lib().mn_bitconv_supported(C.byref(g)):
            raise _err("wbwtab_compile_bits: %s.conv: geometry not covered by mn_bitconv_supported (%dx%d, padding %d, groups %d)" % (nm, k, conv.kernel_size[1], pad, conv.groups))
        if shuffle:
            _check_shuffle_divides("wbwtab_compile_bits", nm, conv, shuffle)
            if not layers:
                raise _err("wbwtab_compile_bits: %s: a channel shuffle directly behind the first block is not covered (its producer is not a bit block)" % nm)
            layers[-1]["shuffle"] = shuffle          # folded into the producer's row order
        layers.append(dict(name=nm, conv=conv, k=k, pad=pad, cin=conv.in_channels, cout=conv.out_channels, groups=conv.groups, pool=0, pool_ksp=None, shuffle=0, stage=name))
        if mfma_blocks:
            layers[-1]["mfma"] = bool(_lib.get_lib().mn_bitconv_mfma_supported(C.byref(g)))
        if mfma_k3:
            layers[-1]["mfma3"] = bool(_lib.get_lib().mn_bitconv_mfma3_supported(C.byref(g)))
    if first is None or last is None:
        raise _err("wbwtab_compile_bits: module order not recognised (no %s conv block found)" % ("first" if first is None else "last"))
    rep_last = report.pop()
    if bit_ends:
        _check_bit_ends(first, report[0]["name"], last, rep_last["name"])
        report[0]["kernel"], rep_last["kernel"] = "first conv -> bits (k_c1b_fwd)", "last conv on bits (k_bitsconv1x1_small)"
    for L in layers:
        # (known only now: the walk folds a pool into the layer after it has passed the block)
        if mfma_blocks and L["pool"] == 2:          # the 3x3 / 2 fold stays on k_bitconv1_pool3
            L["mfma"] = False
        if mfma_k3 and L["pool"]:                   # the pooled 3x3 block stays on k_bitconv<3,*,1>
            L["mfma3"] = False
        kern = _conv_kernel_name(L["k"], L["cin"], L["groups"], L["pool"])
        if L.get("mfma"):
            kern = _bitconv_mfma_kernel_name(L["pool"])
        if L.get("mfma3"):
            kern = _bitconv_mfma3_kernel_name()
        pooled = bool(L["pool"])
        if L["pool"] == 2:
            pooled = "folded 3x3/2"
        elif L["pool_ksp"] and not L["pool"]:
            kern, pooled = kern + ", k_bits_maxpool", "standalone"
        report.append(dict(name=L["name"], kind="bit", K=L["cin"] // L["groups"] * L["k"] * L["k"], words=(L["cin"] + 31) // 32, kernel=kern, pooled=pooled,
                           out_order=("shuffle %d" % L["shuffle"]) if L["shuffle"] > 1 else "identity", stage=L["stage"]))
    report.append(rep_last)
    return first, layers, last, tail, flatten, report


def wbwtab_bits_report(model, bit_ends=False, mfma_blocks=False, mfma_k3=False):
    """The ``report`` ``wbwtab_compile_bits(model, bit_ends, mfma_blocks, mfma_k3)`` would carry -- one row per stage: kernel, K, words, how a max-pool behind it is
    done -- from the graph walk alone: no GPU, nothing packed.  Raises like ``wbwtab_compile_bits`` for whatever the bit kernels do not cover.  Under ``mfma_blocks`` /
    ``mfma_k3`` the ``kernel`` of a block on an MFMA form reads ``k_bitconv_mfma<0|1>`` / ``k_bitconv_mfma3<0>``; nothing else in its row changes."""
    return _walk_bits(model, bit_ends, mfma_blocks, mfma_k3)[5]


@torch.no_grad()
def wbwtab_compile_bits(model, bit_ends=False, mfma_blocks=False, mfma_k3=False):
    """``model``: the result of ``wbwtab_model_bn_fuse`` on a pre-quantised W in (2, 3), A = 2 net, on the GPU (the reference's ``nin`` and ``nin_gc``).  Returns a ``BitPlan``
    computing the same function with one bit per hidden activation; ``.report`` lists the stages.  Anything the bit kernels do not cover raises ``MicronetHipError``
    naming the layer -- never a silent byte path (the caller still has ``model``).  ``bit_ends=True``: the first conv writes the first stage's bits in one launch and the
    classifier reads the last stage's bits -- no fp32 map, no int8 codes, no pack / unpack launch; same bits in every stage, same logits (off by default until the gain
    is measured).  ``mfma_blocks=True``: a 1x1 hidden block ``mn_bitconv_mfma_supported`` covers (dense, or whole input words per group; the folded 2x2 pool
    included) is packed and run in its int8-MFMA form (``mn_bitconv_mfma_*``: same bits, thresholds and order, only the contraction differs); a block with the
    3x3 / 2 fold or fewer than 32 channels per group keeps its kernel.  ``mfma_k3=True``: a 3x3 / padding 1 hidden block ``mn_bitconv_mfma3_supported`` covers
    (C / groups % 16 == 0) with no folded pool is packed and run in its int8-MFMA form (``mn_bitconv_mfma3_*``); a pooled 3x3 block keeps ``k_bitconv``, one whose pool
    runs as ``mn_bits_maxpool`` behind it still moves.  Neither flag refuses anything, both compose with ``bit_ends``; the layer dicts gain the keys ``"mfma"`` /
    ``"mfma3"`` under their flag only.  Off by default; with them off nothing changes."""
    from micronet_amd import _lib, ops
    first, layers, last, tail, flatten, report = _walk_bits(model, bit_ends, mfma_blocks, mfma_k3)
    _require_gpu(model, "wbwtab_compile_bits")
    # ---- pack the weight tables (one launch per layer, once per model)
    lib = _lib.get_lib()
    for L in layers:
        conv = L.pop("conv")
        g = _block_geom(L)
        quartet = "mn_bitconv_mfma" if L.get("mfma") else "mn_bitconv_mfma3" if L.get("mfma3") else "mn_bitconv"
        table = torch.empty(int(getattr(lib, quartet + "_table_bytes")(C.byref(g))) // 4, dtype=torch.int32, device=conv.weight.device)
        order = _shuffle_order(L["cout"], L["shuffle"], conv.weight.device) if L["shuffle"] > 1 else None
        w = conv.weight.detach().float().contiguous()
        b = conv.bias.detach().float().contiguous() if conv.bias is not None else None
        ops._call(quartet + "_pack", C.byref(g), ops._p(w), ops._p(b), ops._p(order), ops._p(table), ops._s())
        L["table"], L["out_order"] = table, order
    bad = [(L["name"], int(L["table"][0])) for L in layers]          # (compile time: the one place a host read-back is allowed)
    for nm, nbad in bad:
        if nbad:
            raise _err("wbwtab_compile_bits: %s.conv: %d output channels whose decision is not monotone in the accumulator" % (nm, nbad))
    return BitPlan(first, layers, last, tail, flatten, report, bit_ends)


# ------------------------------------------------------------------------------------------------ code-packed deployment of DoReFa W2A2 nets (csrc/qgemm_codes.h)
CODE_BITS = 2          # the width every kernel is instantiated for: a_bits = w_bits = 2
CODE_WIDTHS = (2, 4)   # ... and the widths of a whole net: W2A2, or W4A4 on the two int8-MFMA blocks alone (csrc/qgemm_codes_mfma.h, csrc/qgemm_codes_mfma3.h)


def pack_codes(t, bits=None):
    """uint8 activation codes [N, C, H, W] (or a QActTensor) -> int32 tensor [N, ceil(C / 32), bits, H, W] of uint32 words: bit c & 31 of plane p in word group c >> 5 is
    bit p of channel c's code.  Bits of a code above ``bits`` are dropped."""
    from micronet_amd import ops
    from micronet_amd.sign_tensor import QActTensor
    if isinstance(t, QActTensor):
        t, bits = t.codes, (t.bits if bits is None else bits)
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and bits is not None and 1 <= int(bits) <= 8):
        raise _err("pack_codes: needs a QActTensor, or a uint8 code tensor [N, C, H, W] on the GPU and its bit width (no CPU fallback)")
    c = t.contiguous()
    N, Cc, H, W = c.shape
    planes = torch.empty((N, (Cc + 31) // 32, int(bits), H, W), dtype=torch.int32, device=c.device)
    ops._call("mn_codes_pack_planes", ops._p(c), N, Cc, H * W, int(bits), ops._p(planes), ops._s())
    return planes


def unpack_codes(planes, C):
    """The inverse of ``pack_codes``: uint8 codes [N, C, H, W]."""
    from micronet_amd import ops
    if not (torch.is_tensor(planes) and planes.is_cuda and planes.dtype == torch.int32 and planes.dim() == 5 and planes.shape[1] == (int(C) + 31) // 32
            and 1 <= planes.shape[2] <= 8):
        raise _err("unpack_codes: needs an int32 plane tensor [N, ceil(C / 32), bits, H, W] on the GPU")
    planes = planes.contiguous()
    N, _, bits, H, W = planes.shape
    out = torch.empty((N, int(C), H, W), dtype=torch.uint8, device=planes.device)
    ops._call("mn_codes_unpack_planes", ops._p(planes), N, int(C), H * W, int(bits), ops._p(out), ops._s())
    return out


def _codeconv_kernel_name(k, cin, groups, pool):
    """The kernel mn_codeconv_fwd launches for a hidden block (csrc/qgemm_codes.h: nw_select)."""
    cg = cin // groups
    nw = max(((gi * cg + cg - 1) >> 5) - ((gi * cg) >> 5) + 1 for gi in range(groups))
    sel = nw if (nw == 1 or (k == 1 and nw in (2, 4))) else 0
    return "k_codeconv<%d,%d,%d>" % (k, sel, pool)


def _codeconv_mfma_kernel_name(pool):
    """The kernel mn_codeconv_mfma_fwd reports for a 1x1 hidden block (csrc/qgemm_codes_mfma.h)."""
    return "k_codeconv_mfma<%d>" % pool


def _codeconv_mfma3_kernel_name():
    """The kernel mn_codeconv_mfma3_fwd reports for a 3x3 hidden block (csrc/qgemm_codes_mfma3.h)."""
    return "k_codeconv_mfma3<0>"


def _codeconv_tile_kernel_name(k, cin):
    """The kernel mn_codeconv_tile_fwd launches for a dense 5x5 block (csrc/qgemm_codes.h: three word groups unrolled, anything else rolled)."""
    return "k_codeconv_tile<%d,%d>" % (k, 3 if (cin + 31) // 32 == 3 else 0)


class CodePlan(_Plan):
    """What ``dorefa_compile_codes`` returns: first block (fp32 conv + BatchNorm + ReLU + the next conv's quantizer, the model's own module) -> plane pack -> n
    code blocks (2x2 max-pools folded in; with ``tile_blocks`` also the dense 5x5 block on an LDS tile, and a max-pool that ``prepare()`` did not fuse run on the planes
    behind its block) -> plane unpack -> last block and tail (the model's own modules).  Eval only; owns the packed weight tables (and the
    per-channel constants they were packed from: ``layers[i]["chan"]``) and one set of plane buffers per input shape.  ``code_ends``: the first conv's kernel writes
    the first stage's planes itself (no fp32 map, no byte codes, no pack; ``first_table`` holds its per-channel thresholds) and the last conv reads the last stage's
    planes (no unpack, no uint8 buffer); what follows the last conv inside its block, and the tail, run unchanged.  ``bits``: the net's code width, 2 or 4 --
    planes per word group in every buffer, the width of pack / unpack and of the codes handed to the last block; a 4-bit plan holds MFMA blocks only and no
    ``code_ends``."""

    who = "dorefa_compile_codes"

    def __init__(self, first, layers, last, tail, flatten, report, code_ends=False, first_table=None, first_chan=None, bits=2):
        super().__init__(first, layers, last, tail, flatten, report)          # layers: dicts of geometry, table, chan, pool, out_order
        self.code_ends = bool(code_ends)
        self.bits = int(bits)
        if self.bits not in CODE_WIDTHS or (self.bits != CODE_BITS and (self.code_ends or not all(L.get("mfma") or L.get("mfma3") for L in layers))):
            raise _err("dorefa_compile_codes: a %d-bit plan is not covered (2-bit codes, or 4-bit codes on the int8-MFMA blocks alone and without code_ends)" % self.bits)
        self.first_table, self.first_chan = first_table, first_chan
        self.stage_codes = []

    def _plan_buffers(self, shape, device):
        """Plane buffers (and the uint8 buffer in front of the last block) for one first-block output shape."""
        from micronet_amd import _lib
        N, Cc, H, W = shape
        B = self.bits
        g0 = None
        if self.code_ends:
            conv = self.first.conv
            g0 = _conv_geom(conv, N, H, W)          # (Cc is conv.out_channels: forward hands over the first conv's own output shape)
            if not _lib.get_lib().mn_conv2d_first_codes_supported(C.byref(g0), CODE_BITS):
                raise _err("dorefa_compile_codes(code_ends=True): %s.conv: a %d x %d x %d x %d input is not covered by mn_conv2d_first_codes (W %% 4 == 0, H * W %% 32 == 0, "
                           "the image strip in LDS)" % (self.report[0]["name"], N, conv.in_channels, H, W))
        elif (H * W) % 4:
            raise _err("dorefa_compile_codes: %s: its %d x %d output cannot be packed (mn_codes_pack_planes needs H * W %% 4 == 0)" % (self.report[0]["name"], H, W))
        bufs, geoms, mids = [torch.empty((N, (Cc + 31) // 32, B, H, W), dtype=torch.int32, device=device)], [], []
        for L in self.layers:
            geoms.append(_block_geom(L, N, H, W))
            if L["pool"]:
                if H % 2 or W % 2:
                    raise _err("dorefa_compile_codes: %s: the 2x2 max-pool behind it does not fit a %d x %d map" % (L["name"], H, W))
                H, W = H // 2, W // 2
            ksp = L.get("pool_ksp")          # (tile_blocks) a pool the block does not fold: the block at full size into a mid buffer, then mn_codes_maxpool
            if ksp:
                if min(H, W) + 2 * ksp[2] < ksp[0]:
                    raise _err("dorefa_compile_codes: %s: the max-pool behind it does not fit a %d x %d map" % (L["name"], H, W))
                mids.append(torch.empty((N, (L["cout"] + 31) // 32, B, H, W), dtype=torch.int32, device=device))
                H, W = (H + 2 * ksp[2] - ksp[0]) // ksp[1] + 1, (W + 2 * ksp[2] - ksp[0]) // ksp[1] + 1
            else:
                mids.append(None)
            bufs.append(torch.empty((N, (L["cout"] + 31) // 32, B, H, W), dtype=torch.int32, device=device))
            Cc = L["cout"]
        if self.code_ends:
            if not _lib.get_lib().mn_planesconv1x1_small_supported(Cc, H * W, self.last.conv.out_channels, CODE_BITS):
                raise _err("dorefa_compile_codes(code_ends=True): %s.conv: a %d-channel %d x %d map is not covered by mn_planesconv1x1_small_fwd (its lanes own 4 "
                           "consecutive pixels: H * W %% 4 == 0; the weights in LDS)" % (self.report[-1]["name"], Cc, H, W))
            return (bufs, geoms, None, g0, mids)
        if (H * W) % 4:
            raise _err("dorefa_compile_codes: %s: its %d x %d output cannot be unpacked for the last block (mn_codes_unpack_planes needs H * W %% 4 == 0)"
                       % (self.layers[-1]["name"], H, W))
        return (bufs, geoms, torch.empty((N, Cc, H, W), dtype=torch.uint8, device=device), g0, mids)

    def _run_layers(self, bufs, geoms, mids, st):
        """One launch per hidden block (two where a max-pool runs on the planes behind it)."""
        from micronet_amd import ops
        B = self.bits
        for i, L in enumerate(self.layers):
            out = bufs[i + 1] if mids[i] is None else mids[i]
            if L.get("tile"):
                ops._call("mn_codeconv_tile_fwd", C.byref(geoms[i]), ops._p(L["table"]), ops._p(bufs[i]), ops._p(out), st)
            elif L.get("mfma"):
                ops._call("mn_codeconv_mfma_fwd_bits", C.byref(geoms[i]), B, B, B, ops._p(L["table"]), ops._p(bufs[i]), ops._p(out), int(L["pool"]), st)
            elif L.get("mfma3"):
                ops._call("mn_codeconv_mfma3_fwd_bits", C.byref(geoms[i]), B, B, B, ops._p(L["table"]), ops._p(bufs[i]), ops._p(out), 0, st)
            else:
                ops._call("mn_codeconv_fwd", C.byref(geoms[i]), ops._p(L["table"]), ops._p(bufs[i]), ops._p(out), int(L["pool"]), st)
            if mids[i] is not None:
                m, (pk, ps, pp) = mids[i], L["pool_ksp"]
                ops._call("mn_codes_maxpool", ops._p(m), m.shape[0], m.shape[1], B, m.shape[3], m.shape[4], pk, ps, pp, ops._p(bufs[i + 1]), st)

    @torch.no_grad()
    def forward(self, x):
        from micronet_amd import ops
        from micronet_amd.sign_tensor import QActTensor
        if self.code_ends:
            conv = self.first.conv
            if not (type(x) is torch.Tensor and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == conv.in_channels):
                raise _err("dorefa_compile_codes(code_ends=True): the input must be a float32 GPU tensor [N, %d, H, W] (no CPU fallback)" % conv.in_channels)
            x = x.contiguous()
            with torch.cuda.device(x.device):
                bufs, geoms, c8, g0, mids = self._shape_buffers((x.shape[0], conv.out_channels, x.shape[2], x.shape[3]), x.device)
                st = ops._s()
                ops._call("mn_conv2d_first_codes", C.byref(g0), ops._p(x), ops._p(ops._chk(conv.weight.detach(), "weight")), ops._p(ops._chk(conv.bias, "bias")),
                          ops._p(self.first_table), ops._p(bufs[0]), st)
                self._run_layers(bufs, geoms, mids, st)
                if self.keep_stages:
                    self.stage_codes = [b.clone() for b in bufs]
                conv = self.last.conv
                n_, _, _, h_, w_ = bufs[-1].shape
                y = torch.empty((n_, conv.out_channels, h_, w_), dtype=torch.float32, device=x.device)
                ops._call("mn_planesconv1x1_small_fwd", ops._p(bufs[-1]), CODE_BITS, ops._p(ops._chk(conv.weight.detach(), "weight")), ops._p(ops._chk(conv.bias, "bias")),
                          ops._p(y), n_, conv.in_channels, h_ * w_, conv.out_channels, st)
            return self._finish(self._after_conv(self.last, conv, y))          # (BatchNorm + ReLU)
        B = self.bits
        a = self.first(x)
        if not (isinstance(a, QActTensor) and a.bits == B):
            raise _err("dorefa_compile_codes: %s did not hand over %d-bit activation codes (the input must be a contiguous float32 GPU tensor with H * W %% 8 == 0)"
                       % (self.report[0]["name"], B))
        codes = a.codes.contiguous()
        N, Cc, H, W = codes.shape
        bufs, geoms, c8, _, mids = self._shape_buffers(codes.shape, codes.device)
        st = ops._s()
        ops._call("mn_codes_pack_planes", ops._p(codes), N, Cc, H * W, B, ops._p(bufs[0]), st)
        self._run_layers(bufs, geoms, mids, st)
        if self.keep_stages:
            self.stage_codes = [b.clone() for b in bufs]
        n_, c_, h_, w_ = c8.shape
        ops._call("mn_codes_unpack_planes", ops._p(bufs[-1]), n_, c_, h_ * w_, B, ops._p(c8), st)
        # (materialize: a consumer that does not read codes re-quantises 10 j s to j -- the middle of the code's bin)
        return self._finish(self.last(QActTensor(c8, B, lambda: c8.float() * (10.0 / (2 ** B - 1)))))


def _check_code_ends(first, nm_first, last, nm_last):
    """``code_ends=True``: ``_check_ends`` for the two plane kernels, and no channel shuffle in front of the last conv (the walk has already refused a pool behind the
    first block, other than 2-bit codes out of it, and a block's shuffle in front of the last block)."""
    from micronet_amd import _lib
    lib = _lib.get_lib()
    _check_ends("dorefa_compile_codes(code_ends=True)", first, nm_first, last, nm_last, "mn_conv2d_first_codes",
                lambda g: lib.mn_conv2d_first_codes_supported(C.byref(g), CODE_BITS), "mn_planesconv1x1_small_fwd",
                lambda cin, hw, cout: lib.mn_planesconv1x1_small_supported(cin, hw, cout, CODE_BITS))
    if getattr(last, "channel_shuffle_flag", 0) and getattr(last, "shuffle_groups", 1) > 1 or int(getattr(last.conv, "in_shuffle_groups", 0) or 0) > 1:
        raise _err("dorefa_compile_codes(code_ends=True): %s: a channel shuffle in front of the last conv is not covered by mn_planesconv1x1_small_fwd" % nm_last)


def _walk_codes(model, code_ends=False, tile_blocks=False, mfma_blocks=False, mfma_k3=False):
    """The graph walk of ``dorefa_compile_codes`` (no GPU needed): (first, layers, last, tail, flatten, report).  ``tile_blocks``: also admit what plain nin needs -- a
    dense 5x5 block (``layer["tile"]``) and a max-pool ``prepare()`` did not fuse, run on the planes behind its block (``layer["pool_ksp"]``).  ``mfma_blocks``: a
    hidden block ``mn_codeconv_mfma_supported`` covers runs on the MFMA form (``layer["mfma"]``); it refuses nothing.  ``mfma_k3``: a hidden 3x3 block
    ``mn_codeconv_mfma3_supported`` covers, with no folded pool, runs on the 3x3 MFMA form (``layer["mfma3"]``); it refuses nothing either.  The net's code width is that
    of the first hidden block's conv, W2A2 or W4A4 (``report[i]["planes"]``); every quantised block must have it.  A 4-bit net runs on the two MFMA forms alone, whatever
    the two flags say: a hidden block neither covers, ``code_ends`` and ``tile_blocks`` raise."""
    from micronet_amd import _lib
    from micronet_amd.nn import Conv2dFirst
    from micronet_amd.quantization.wqaq.dorefa import quantize
    seq, prefix, flatten = _net_sequence(model, "dorefa_compile_codes")
    blocks = [(prefix + n_, m) for n_, m in seq.named_children() if quantize._is_ref_block(m) and isinstance(getattr(m, "conv", None), nn.Conv2d)]
    if len(blocks) < 3:
        raise _err("dorefa_compile_codes: module order not recognised (needs a first block, at least one quantised hidden block and a last block)")
    # ---- what the kernels are instantiated for, checked over the whole net first: the error names the layer
    width = None          # (a_bits, w_bits) of the net: the first hidden block's
    for nm, blk in blocks[1:]:
        conv = blk.conv
        if not isinstance(conv, quantize.QuantConv2d):
            raise _err("dorefa_compile_codes: %s.conv is not a DoReFa QuantConv2d" % nm)
        ab, wb = conv.activation_quantizer.a_bits, conv.weight_quantizer.w_bits
        if width is None:
            width = (ab, wb)
        if (ab, wb) != width or ab != wb or ab not in CODE_WIDTHS:
            raise _err("dorefa_compile_codes: %s.conv has a_bits = %d, w_bits = %d; only W2A2 and W4A4 nets are code-packed, every quantised block at the width of the "
                       "first hidden block (here a_bits = %d, w_bits = %d)" % (nm, ab, wb, width[0], width[1]))
        if not conv.quant_inference:
            raise _err("dorefa_compile_codes: %s.conv is not a quant_inference=True layer (prepare(..., quant_inference=True), then prequantize_weights)" % nm)
    B = width[0]
    wide = B != CODE_BITS          # a 4-bit net: the two int8-MFMA forms or nothing
    if wide and code_ends:
        raise _err("dorefa_compile_codes(code_ends=True): %s.conv: the net has %d-bit codes; the first conv's plane epilogue and the classifier on planes are built for "
                   "2 bits only" % (blocks[0][0], B))
    if wide and tile_blocks:
        raise _err("dorefa_compile_codes(tile_blocks=True): %s.conv: the net has %d-bit codes; the 5x5 tile block and the max-pools on planes are built for 2 bits only"
                   % (blocks[1][0], B))
    tiled = set()          # (tile_blocks) the hidden blocks mn_codeconv_tile_* runs
    for nm, blk in blocks[1:-1]:
        conv = blk.conv
        if tuple(conv.stride) != (1, 1) or tuple(conv.dilation) != (1, 1) or conv.padding_mode != "zeros" or isinstance(conv.padding, str):
            raise _err("dorefa_compile_codes: %s.conv: stride / dilation other than 1 (or non-zero padding mode) is not covered by the code kernels" % nm)
        g = _conv_geom(conv)          # (stride and dilation are 1: anything else was refused above)
        if wide:
            if not (_lib.get_lib().mn_codeconv_mfma_supported(C.byref(g), B, B, B) or _lib.get_lib().mn_codeconv_mfma3_supported(C.byref(g), B, B, B)):
                ks, cg, n = tuple(conv.kernel_size), conv.in_channels // conv.groups, 2 ** B - 1
                if ks == (1, 1) and tuple(conv.padding) == (0, 0):
                    why = ("%d channels per group: a grouped 1x1 block needs whole input words per group (C / groups %% 32 == 0)" % cg if conv.groups > 1 and cg % 32
                           else "%d taps per output: beyond K * %d * %d <= 32767, the int16 range the thresholds are searched over (at most %d)" % (cg, n, n, 32767 // (n * n)))
                elif ks == (3, 3) and tuple(conv.padding) == (1, 1):
                    why = "%d channels per group: the 3x3 MFMA form covers C / groups == 16 at %d bits (K = 144, K * %d * %d <= 32767)" % (cg, B, n, n)
                else:
                    why = "%dx%d, padding %d: only the 1x1 and the 3x3 / padding 1 block have a %d-bit form" % (ks[0], ks[1], conv.padding[0], B)
                raise _err("dorefa_compile_codes: %s.conv: not covered by the %d-bit int8-MFMA blocks (mn_codeconv_mfma_supported, mn_codeconv_mfma3_supported), the "
                           "only %d-bit code blocks: %s" % (nm, B, B, why))
            continue
        if not _lib.get_lib().mn_codeconv_supported(C.byref(g), CODE_BITS, CODE_BITS, CODE_BITS):
            five = tuple(conv.kernel_size) == (5, 5)
            if tile_blocks and _lib.get_lib().mn_codeconv_tile_supported(C.byref(g), CODE_BITS, CODE_BITS, CODE_BITS):
                tiled.add(nm)
                continue
            if tile_blocks and five and conv.groups != 1:
                raise _err("dorefa_compile_codes(tile_blocks=True): %s.conv: a grouped 5x5 block (groups %d) is not covered by mn_codeconv_tile_supported (dense only)"
                           % (nm, conv.groups))
            if tile_blocks and five and tuple(conv.padding) == (2, 2):
                raise _err("dorefa_compile_codes(tile_blocks=True): %s.conv: a 5x5 block of %d input channels is beyond the bound of mn_codeconv_tile_supported (C * 25 * 9 <= "
                           "32767: at most 145 channels, the int16 range the thresholds are searched over)" % (nm, conv.in_channels))
            raise _err("dorefa_compile_codes: %s.conv: geometry not covered by mn_codeconv_supported (%dx%d, padding %d, groups %d, %d taps per output: needs 1x1 or 3x3 with "
                       "padding 1, and at most 3640 taps)%s" % (nm, conv.kernel_size[0], conv.kernel_size[1], conv.padding[0], conv.groups,
                                                               conv.in_channels // conv.groups * conv.kernel_size[0] * conv.kernel_size[1],
                                                               "; tile_blocks=True admits the dense 5x5 / padding 2 block of plain nin" if five and not tile_blocks else ""))
    first = last = None
    layers, tail, report = [], [], []
    kids = list(seq.named_children())
    pending = None          # (tile_blocks) the standalone pool the walk has just passed: a quantised block must follow
    for ki, (name, child) in enumerate(kids):
        nm = prefix + name
        if last is not None:
            tail.append(child)
            continue
        if tile_blocks and isinstance(child, nn.MaxPool2d) and not getattr(child, "_mn_fused_pool", False):
            # ---- a max-pool prepare() did not fuse into the block in front of it: run on that block's planes (mn_codes_maxpool)
            ksp = _pool_kind(child)
            if ksp is None:
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: max-pool (kernel %s, stride %s, padding %s, ceil_mode %s) is not covered by the code kernels "
                           "(2x2 / 2 / 0 and 3x3 / 2 / 1, floor mode)" % (nm, child.kernel_size, child.stride, child.padding, child.ceil_mode))
            if pending is not None or (layers and (layers[-1]["pool"] or layers[-1].get("pool_ksp"))):
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: two max-pools in a row are not covered (one pool behind a code block)" % nm)
            if not layers:
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: a max-pool directly behind the first block is not covered (its producer is not a code block)" % nm)
            if not layers[-1]["wants_consumer"]:
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: the block in front of this max-pool already hands its codes to another consumer" % nm)
            layers[-1]["wants_consumer"], layers[-1]["pool_ksp"], layers[-1]["stage"] = False, ksp, name
            pending = nm
            continue
        if isinstance(child, nn.MaxPool2d):
            if _pool_kind(child) != (2, 2, 0):
                raise _err("dorefa_compile_codes: %s: max-pool (kernel %s, stride %s, padding %s, ceil_mode %s) is not covered by the code kernels (2x2 / 2 / 0, floor mode)"
                           % (nm, child.kernel_size, child.stride, child.padding, child.ceil_mode))
            if not layers or layers[-1]["pool"] or not getattr(child, "_mn_fused_pool", False):
                raise _err("dorefa_compile_codes: %s: a 2x2 max-pool is folded only into the code block directly in front of it" % nm)
            layers[-1]["pool"], layers[-1]["stage"] = 1, name
            continue
        if not any(child is b for _, b in blocks):
            raise _err("dorefa_compile_codes: %s (%s): module order not recognised (expected conv -> bn -> relu blocks and 2x2 max-pools up to the last block)"
                       % (nm, type(child).__name__))
        conv, bn = child.conv, getattr(child, "bn", None)
        if not isinstance(bn, quantize.BatchNorm2dReLU):
            raise _err("dorefa_compile_codes: %s: conv -> BatchNorm -> ReLU not fused (prepare(..., fuse_bn_act=True, fuse_blocks=True))" % nm)
        if pending is not None:          # the consumer of a standalone pool: its activation quantizer is the one the producer's thresholds stand for
            if not isinstance(conv, quantize.QuantConv2d) or conv.activation_quantizer.a_bits != CODE_BITS:
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: the block behind the max-pool %s must be a quantised conv reading %d-bit codes" % (nm, pending, CODE_BITS))
            pending = None
        K = conv.in_channels // conv.groups * conv.kernel_size[0] * conv.kernel_size[1]
        if first is None:
            if type(conv) is not Conv2dFirst or getattr(child, "channel_shuffle_flag", 0):
                raise _err("dorefa_compile_codes: %s: the first block must be the fp32 first conv" % nm)
            if tile_blocks and not bn.q_out_bits and ki + 1 < len(kids) and isinstance(kids[ki + 1][1], nn.MaxPool2d):
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: a max-pool directly behind the first block is not covered (its producer, %s, is not a code block)"
                           % (prefix + kids[ki + 1][0], nm))
            if bn.q_out_bits != B:
                raise _err("dorefa_compile_codes: %s: the first block must hand over %d-bit activation codes (it emits %s)"
                           % (nm, B, ("%d-bit codes" % bn.q_out_bits) if bn.q_out_bits else "fp32"))
            if bn.q_pool:
                raise _err("dorefa_compile_codes: %s: a 2x2 max-pool is folded only into a code block; directly behind the first block it is not covered" % nm)
            first = child
            report.append(dict(name=nm, kind="first", K=K, words=0, planes=0, kernel="first conv + k_qa_fwd, k_codes_pack", pooled=False, out_order="identity", stage=name))
            continue
        shuffle = _shuffle_in_front("dorefa_compile_codes", nm, child, conv)
        if child is blocks[-1][1]:
            if shuffle:
                raise _err("dorefa_compile_codes: %s: a channel shuffle in front of the last block is not covered" % nm)
            last = child
            report.append(dict(name=nm, kind="last", K=K, words=(conv.in_channels + 31) // 32, planes=B, kernel="k_codes_unpack, last block on byte codes",
                               pooled=False, out_order="identity", stage=name))
            continue
        # ---- a hidden block: conv on codes -> bn -> relu -> [pool] -> the next conv's quantizer
        wants = False
        if tile_blocks and not bn.q_out_bits and ki + 1 < len(kids) and isinstance(kids[ki + 1][1], nn.MaxPool2d) and not getattr(kids[ki + 1][1], "_mn_fused_pool", False):
            # prepare() left the block emitting fp32 because an un-fused max-pool follows: it emits the codes of the conv behind that pool instead (checked when the
            # walk gets there) -- exact, the pool sits behind the ReLU and the quantizer is non-decreasing
            wants = True
        elif bn.q_out_bits != B:
            raise _err("dorefa_compile_codes: %s: its output is not handed over as %d-bit codes to the next quantised conv" % (nm, B))
        if shuffle:
            _check_shuffle_divides("dorefa_compile_codes", nm, conv, shuffle)
            if not layers:
                raise _err("dorefa_compile_codes: %s: a channel shuffle directly behind the first block is not covered (its producer is not a code block)" % nm)
            layers[-1]["shuffle"] = shuffle          # folded into the producer's row order
        layers.append(dict(name=nm, conv=conv, bn=bn, k=conv.kernel_size[0], pad=conv.padding[0], cin=conv.in_channels, cout=conv.out_channels, groups=conv.groups,
                           pool=0, want_pool=bool(bn.q_pool), shuffle=0, stage=name))
        if tile_blocks:
            layers[-1].update(tile=nm in tiled, pool_ksp=None, wants_consumer=wants)
        if mfma_blocks or mfma_k3 or wide:
            g = _conv_geom(conv)
            if mfma_blocks or wide:
                layers[-1]["mfma"] = bool(_lib.get_lib().mn_codeconv_mfma_supported(C.byref(g), B, B, B))
            if mfma_k3 or wide:
                layers[-1]["mfma3"] = bool(_lib.get_lib().mn_codeconv_mfma3_supported(C.byref(g), B, B, B))
    if pending is not None:
        raise _err("dorefa_compile_codes(tile_blocks=True): %s: no quantised block behind this max-pool" % pending)
    if first is None or last is None:
        raise _err("dorefa_compile_codes: module order not recognised (no %s block found)" % ("first" if first is None else "last"))
    rep_last = report.pop()
    if code_ends:
        _check_code_ends(first, report[0]["name"], last, rep_last["name"])
        report[0]["kernel"], rep_last["kernel"] = "first conv -> planes (k_c1b_fwd)", "last conv on planes (k_planesconv1x1_small)"
    for L in layers:
        if L.pop("want_pool") != bool(L["pool"]):
            raise _err("dorefa_compile_codes: %s: the block pools its output but no 2x2 max-pool follows it (or the reverse)" % L["name"])
        kern, pooled = _codeconv_kernel_name(L["k"], L["cin"], L["groups"], L["pool"]), bool(L["pool"])
        if wide and L["mfma3"] and L["pool"]:
            raise _err("dorefa_compile_codes: %s.conv: a 3x3 block with a folded 2x2 max-pool is not covered at %d bits (no pool is folded into the 3x3 MFMA form, the "
                       "only %d-bit 3x3 block)" % (L["name"], B, B))
        if mfma_k3 and L["pool"]:          # (known only now: the walk folds a 2x2 pool into the layer after it has passed the block)
            L["mfma3"] = False
        if tile_blocks:
            if L.pop("wants_consumer"):
                raise _err("dorefa_compile_codes(tile_blocks=True): %s: its output is not handed over as %d-bit codes to the next quantised conv" % (L["name"], CODE_BITS))
            if L["tile"]:
                kern = _codeconv_tile_kernel_name(L["k"], L["cin"])
        if L.get("mfma"):
            kern = _codeconv_mfma_kernel_name(L["pool"])
        if L.get("mfma3"):
            kern = _codeconv_mfma3_kernel_name()
        if tile_blocks:          # (behind the block's own kernel name, whichever it is)
            if L["pool_ksp"]:
                kern, pooled = kern + ", k_codes_maxpool", "standalone"
        report.append(dict(name=L["name"], kind="code", K=L["cin"] // L["groups"] * L["k"] * L["k"], words=(L["cin"] + 31) // 32, planes=B,
                           kernel=kern, pooled=pooled,
                           out_order=("shuffle %d" % L["shuffle"]) if L["shuffle"] > 1 else "identity", stage=L["stage"]))
    report.append(rep_last)
    return first, layers, last, tail, flatten, report


def dorefa_codes_report(model, code_ends=False, tile_blocks=False, mfma_blocks=False, mfma_k3=False):
    """The ``report`` ``dorefa_compile_codes(model, code_ends)`` would carry -- one row per stage: name, kind, K, words, planes, kernel, pooled, out_order -- from the
    graph walk alone: no GPU, nothing packed.  Raises like ``dorefa_compile_codes`` for whatever the code kernels do not cover.  ``tile_blocks`` as there: a block on
    ``k_codeconv_tile`` is named so, a max-pool run on the planes behind its block reads ``pooled="standalone"`` and ``"<block kernel>, k_codes_maxpool"``.
    ``mfma_blocks`` as there: the ``kernel`` of a block on the MFMA form reads ``k_codeconv_mfma<0|1>``.  ``mfma_k3`` as there: a 3x3 block on its MFMA form reads
    ``k_codeconv_mfma3<0>``.  A W4A4 net (the width is the first hidden block's) reads ``planes = 4`` and the two MFMA kernels in every hidden row, with or without the
    two flags; ``code_ends`` / ``tile_blocks`` and a block neither MFMA form covers raise."""
    return _walk_codes(model, code_ends, tile_blocks, mfma_blocks, mfma_k3)[5]


def _bn_chan_constants(bn, O, gamma, beta):
    """The [9][O] constants of an eval-mode BatchNorm + quantizer on an fp32 map, by the calls its eval forward makes (ops._bn_front: mn_bn_save_stats with training = 0,
    mn_qa_chan_from_save -- invstd is never re-derived here).  They do not depend on the input, so one 8 x 8 map of zeros will do."""
    from micronet_amd import _lib, ops
    dev = gamma.device
    zero = torch.zeros((1, O, 8, 8), dtype=torch.float32, device=dev)
    save = torch.empty((2, O), dtype=torch.float32, device=dev)
    chan = torch.empty((_lib.MN_QA_NCH, O), dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.get_lib().mn_bnsign_ws_floats(O)), dtype=torch.float32, device=dev)
    ops._call("mn_bn_save_stats", ops._p(zero), 1, O, 64, float(bn.eps), float(bn.momentum), 0, ops._p(bn.running_mean), ops._p(bn.running_var), ops._p(save), ops._p(ws), ops._s())
    ops._call("mn_qa_chan_from_save", ops._p(save), ops._p(gamma), ops._p(beta), O, ops._p(chan), ops._s())
    return chan


@torch.no_grad()
def dorefa_compile_codes(model, code_ends=False, tile_blocks=False, mfma_blocks=False, mfma_k3=False):
    """``model``: a DoReFa W2A2 (or W4A4: last paragraph) net prepared with ``quant_inference=True`` after ``prequantize_weights``, on the GPU (the reference's ``nin_gc``, or an ``nn.Sequential``
    of the same block kinds).  Returns a ``CodePlan`` computing the same function with two bits per hidden activation; ``.report`` lists the stages.  Anything the code
    kernels do not cover raises ``MicronetHipError`` naming the layer -- never a silent byte path (the caller still has ``model``).  ``code_ends=True``: the first conv
    writes the first stage's planes in one launch and the classifier reads the last stage's planes -- no fp32 map, no byte codes, no pack / unpack launch; same codes
    in every stage, same logits (off by default until the gain is measured).  ``tile_blocks=True``: also admits what plain ``nin`` needs -- a dense 5x5 / padding 2 block
    of at most 145 input channels on an LDS-resident tile (``mn_codeconv_tile_*``), and a 2x2 / 2 or 3x3 / 2 / 1 max-pool ``prepare()`` did not fuse, directly behind a
    hidden block and in front of a quantised one, run on the planes (``mn_codes_maxpool``; the block in front emits the codes of the conv behind the pool: exact, the
    pool sits behind the ReLU and the quantizer is non-decreasing).  Off by default; with it off nothing changes.  ``mfma_blocks=True``: a 1x1 hidden block
    ``mn_codeconv_mfma_supported`` covers (dense, or at least 32 channels per group on word boundaries; the folded 2x2 pool included) is packed and run in its
    int8-MFMA form (``mn_codeconv_mfma_*``: same planes, thresholds and bits, only the contraction differs); every other block keeps what it has, nothing is refused
    on its account, and it composes with the other two flags.  The layer dicts gain the key ``"mfma"``.  Off by default; with it off nothing changes.
    ``mfma_k3=True``: a 3x3 / padding 1 hidden block ``mn_codeconv_mfma3_supported`` covers (C / groups % 16 == 0, at most 400 channels per group) with no folded pool
    is packed and run in its int8-MFMA form (``mn_codeconv_mfma3_*``: an implicit GEMM over (tap, channel), same planes, thresholds and bits); a pooled 3x3 block
    and every other block keep what they have, nothing is refused on its account, and it composes with the other three flags.  The layer dicts gain the key
    ``"mfma3"``.  Off by default; with it off nothing changes.

    A W4A4 net -- every quantised block at ``a_bits = w_bits = 4``, the width read off the first hidden block -- is compiled the same way into a plan with four bits
    per hidden activation (``plan.bits == 4``, ``report[i]["planes"] == 4``).  At 4 bits only the two int8-MFMA forms exist, so both are selected whatever
    ``mfma_blocks`` / ``mfma_k3`` say and the layer dicts carry ``"mfma"`` / ``"mfma3"``: a 1x1 block must be dense with at most 145 input channels or have 32, 64, 96
    or 128 channels per group, a 3x3 / padding 1 block 16 channels per group and no folded pool (K * 15 * 15 <= 32767, the int16 range the thresholds are searched
    over).  Any other hidden block, ``code_ends=True`` and ``tile_blocks=True`` raise ``MicronetHipError`` naming the layer; so does a net of mixed widths or of any
    other width.  The stored weights must lie on the 4-bit grid (2k - 15) / 15.  Nothing changes for a W2A2 net."""
    from micronet_amd import _lib, ops
    from micronet_amd.quantization.wqaq.dorefa.quantize import _weight_is_coded
    first, layers, last, tail, flatten, report = _walk_codes(model, code_ends, tile_blocks, mfma_blocks, mfma_k3)
    B = report[-1]["planes"]          # the net's code width: 2 or 4
    for L in layers:
        if not _weight_is_coded(L["conv"]):
            raise _err("dorefa_compile_codes: %s.conv: the stored weights were not found on the %d-bit grid (2k - %d) / %d (run inference.prequantize_weights on the GPU "
                       "model first)" % (L["name"], B, 2 ** B - 1, 2 ** B - 1))
    if code_ends and not _weight_is_coded(last.conv):
        raise _err("dorefa_compile_codes(code_ends=True): %s.conv: the stored weights were not found on the 2-bit grid (2k - 3) / 3 (run inference.prequantize_weights "
                   "on the GPU model first)" % report[-1]["name"])
    _require_gpu(model, "dorefa_compile_codes")
    lib = _lib.get_lib()
    for L in layers:
        conv, bn = L.pop("conv"), L.pop("bn")
        dev = conv.weight.device
        w = conv.weight.detach().float().contiguous()
        b = conv.bias.detach().float().contiguous() if conv.bias is not None else None
        with torch.cuda.device(dev):
            # ---- the [9][O] constants of the block's eval-mode BatchNorm, by the calls the block's eval forward makes (ops._bn_front).  They do not depend on the
            #      input, so one 8 x 8 map of zeros will do.
            if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
                raise _err("dorefa_compile_codes: %s.bn: needs affine parameters, running statistics and a momentum" % L["name"])
            gamma, beta = ops._chk(bn.weight.detach(), "weight"), ops._chk(bn.bias.detach(), "bias")
            g8 = _block_geom(L, 1, 8, 8)
            wd = ops._wq_dorefa(B, None, 0)
            tile = bool(L.get("tile"))
            if not tile and lib.mn_qconv_bnq_supported(C.byref(g8), C.byref(wd), B) and int(lib.mn_qconv_bnq_stash_bits(C.byref(g8), C.byref(wd), B)) == 16:
                # the fused block: the conv on codes with training = 0 writes the constants from the running statistics (alpha = weight scale x activation scale)
                zero = torch.zeros((1, L["cin"], 8, 8), dtype=torch.uint8, device=dev)
                save = torch.empty((2, L["cout"]), dtype=torch.float32, device=dev)
                chan = torch.empty((_lib.MN_QA_NCH, L["cout"]), dtype=torch.float32, device=dev)
                stash = torch.empty((1, L["cout"], 8, 8), dtype=torch.int16, device=dev)
                nb = int(lib.mn_qconv_bnq_ws_bytes(C.byref(g8)))
                ws = torch.empty(nb // 4 + 4, dtype=torch.float32, device=dev)
                ops._call("mn_qconv_bnq_fwd_stash", C.byref(g8), C.byref(wd), ops._p(zero), B, ops._p(w), ops._p(b), ops._p(gamma), ops._p(beta), float(bn.eps),
                          float(bn.momentum), 0, ops._p(bn.running_mean), ops._p(bn.running_var), None, ops._p(save), ops._p(stash), ops._p(chan), ops._p(ws), nb, ops._s())
            else:
                # a block the stash conv does not cover (narrow groups) -- and, by the same route, the tiled 5x5 block: its eval forward convolves to fp32
                # y = acc * alpha + bias (the code kernels' epilogue) and
                # takes (mean, invstd) from mn_bn_save_stats -- the same two calls here; rows alpha / bias (1 / 0 for an fp32 input) become the epilogue's
                chan = _bn_chan_constants(bn, L["cout"], gamma, beta)
                sc = torch.tensor(1.0 / (2 ** B - 1), dtype=torch.float32, device=dev)
                chan[0] = sc * sc          # fp32 product of the weight and the activation scale, as k_qa_stats_prep forms it
                chan[1] = b if b is not None else 0.0
                chan[6], chan[7] = chan[0] * chan[3], (chan[1] - chan[2]) * chan[3]
            # ---- the table (one launch per layer, once per model)
            g = _block_geom(L)
            quartet = "mn_codeconv_tile" if tile else "mn_codeconv_mfma" if L.get("mfma") else "mn_codeconv_mfma3" if L.get("mfma3") else "mn_codeconv"
            table = torch.empty(int(getattr(lib, quartet + "_table_bytes")(C.byref(g), B, B, B)) // 4, dtype=torch.int32, device=dev)
            order = _shuffle_order(L["cout"], L["shuffle"], dev) if L["shuffle"] > 1 else None
            ops._call(quartet + "_pack", C.byref(g), ops._p(w), ops._p(chan), B, B, B, ops._p(order), ops._p(table), ops._s())
        L["table"], L["chan"], L["out_order"] = table, chan, order
    for L in layers:          # (compile time: the one place a host read-back is allowed)
        nonfinite, bad = int(L["table"][0]), int(L["table"][7])
        if nonfinite:
            raise _err("dorefa_compile_codes: %s.bn: %d output channels with a non-finite (or beyond 1e9) BatchNorm constant: no integer thresholds" % (L["name"], nonfinite))
        if bad:
            raise _err("dorefa_compile_codes: %s.conv: %d table rows with a weight off the %d-bit grid or a bad channel order" % (L["name"], bad, B))
    if not code_ends:
        return CodePlan(first, layers, last, tail, flatten, report, bits=B)
    # ---- the first block's per-channel thresholds, from its [9][O] constants
    bn, nm = first.bn, report[0]["name"]
    if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
        raise _err("dorefa_compile_codes(code_ends=True): %s.bn: needs affine parameters, running statistics and a momentum" % nm)
    dev, Oc = first.conv.weight.device, first.conv.out_channels
    with torch.cuda.device(dev):
        chan = _bn_chan_constants(bn, Oc, ops._chk(bn.weight.detach(), "weight"), ops._chk(bn.bias.detach(), "bias"))
        table = torch.empty(int(lib.mn_conv2d_first_codes_table_bytes(Oc, CODE_BITS)) // 4, dtype=torch.int32, device=dev)
        ops._call("mn_conv2d_first_codes_pack", ops._p(chan), Oc, CODE_BITS, ops._p(table), ops._s())
    nonfinite = int(table[0])          # (compile time: read back once)
    if nonfinite:
        raise _err("dorefa_compile_codes(code_ends=True): %s.bn: %d output channels with a non-finite (or beyond 1e9) BatchNorm constant: no thresholds" % (nm, nonfinite))
    return CodePlan(first, layers, last, tail, flatten, report, code_ends=True, first_table=table, first_chan=chan)


# ------------------------------------------------------------------------------------------------ int8 deployment of the BN-folded IAO graph (csrc/qgemm_iao8.h)
def _i8conv_kernel_name(k, pool, zp=False):
    """The kernel mn_i8conv_fwd reports for a hidden block (csrc/qgemm_iao8.h); ``zp``: mn_i8zconv_fwd, for a block with a zero point (csrc/qgemm_iao8_zp.h)."""
    return ("k_i8zconv<%d,%d>" if zp else "k_i8conv<%d,%d>") % (k, pool)


def _blocked(c, h, w):
    """The bytes of a code map of c channels on an h x w map: whole 16-channel blocks."""
    return (c + 15) // 16 * 16 * h * w


def _code_map(N, c, hw, device, fill=None):
    """A blocked code map [N, ceil(c / 16), hw, 16] of int8; ``fill``: the poison of a map handed to the tests."""
    shape = (N, (c + 15) // 16, hw, 16)
    return torch.empty(shape, dtype=torch.int8, device=device) if fill is None else torch.full(shape, fill, dtype=torch.int8, device=device)


def _is_code_map(t, N, c, hw):
    """An int8 GPU tensor of the shape ``_code_map`` makes for c channels."""
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int8 and tuple(t.shape) == (N, (c + 15) // 16, hw, 16)


def _iao8_check_quantizer(q, nm, per_tensor, who="iao_compile_int8", zero_points=False):
    """A quantizer the int8 blocks cover: symmetric (zero point 0), 2 .. 8 bits; ``per_tensor``: exactly one scale.  ``zero_points``: an ``AsymmetricQuantizer`` is
    covered as well (``per_tensor``: exactly one zero point), its ``q_type`` attribute agreeing with its class.  Returns 1 for an asymmetric quantizer, else 0."""
    from micronet_amd.quantization.wqaq.iao import quantize
    if not isinstance(q, quantize.Quantizer):
        raise _err("%s: %s is not an IAO quantizer" % (who, nm))
    if q.bits == 32 or not 2 <= q.bits <= 8:
        raise _err("%s: %s has %d bits; the int8 blocks cover code widths 2 .. 8" % (who, nm, q.bits))
    if zero_points and q.q_type != q._q_type_static:
        raise _err("%s: %s (%s) carries q_type %s, its class q_type %d: the quantizer never updated its parameters, or the attribute was changed"
                   % (who, nm, type(q).__name__, q.q_type, q._q_type_static))
    asym = int(zero_points and q._q_type_static == 1)
    if not asym and (q._q_type_static != 0 or q.q_type != 0 or bool((q.zero_point != 0).any())):
        raise _err("%s: %s is asymmetric; a zero byte must be the value 0 (symmetric quantizers only)" % (who, nm))
    if per_tensor and q.scale.numel() != 1:
        raise _err("%s: %s carries %d scales; a per-tensor activation scale must be a single value" % (who, nm, q.scale.numel()))
    if asym and per_tensor and q.zero_point.numel() != 1:
        raise _err("%s: %s carries %d zero points; a per-tensor activation zero point must be a single value" % (who, nm, q.zero_point.numel()))
    return asym


def _iao8_check_conv(conv, nm, who="iao_compile_int8", zero_points=False, fold_only=False):
    """A conv the int8 blocks deploy: a BN-folded IAO ``QuantConv2d`` that is ``quant_inference``, its activation quantizer covered with a single scale.  ``nm``,
    here and in ``_iao8_check_weights``: the conv's own path in the model.  ``fold_only``: the first rule alone, for a conv that stays on the model's own module."""
    from micronet_amd.quantization.wqaq.iao import quantize
    if not isinstance(conv, quantize.QuantConv2d) or isinstance(conv, quantize.QuantBNFuseConv2d):
        raise _err("%s: %s (%s) is not a BN-folded IAO QuantConv2d (run iao_model_bn_fuse first)" % (who, nm, type(conv).__name__))
    if fold_only:
        return
    if not conv.quant_inference:
        raise _err("%s: %s is not quant_inference: its stored weights are not on the grid (iao_model_bn_fuse + prequantize_weights)" % (who, nm))
    _iao8_check_quantizer(conv.activation_quantizer, nm + ".activation_quantizer", True, who, zero_points)


def _iao8_check_weights(conv, nm, who="iao_compile_int8", zero_points=False):
    """The weight quantizer and padding mode of a conv the int8 blocks contract: symmetric (``zero_points``: or asymmetric, as many zero points as scales), 2 .. 8
    bits, one scale per layer or per output channel, zero padding."""
    wq = conv.weight_quantizer
    asym = _iao8_check_quantizer(wq, nm + ".weight_quantizer", False, who, zero_points)
    if asym and wq.zero_point.numel() != wq.scale.numel():
        raise _err("%s: %s.weight_quantizer carries %d zero points for %d scales" % (who, nm, wq.zero_point.numel(), wq.scale.numel()))
    if wq.scale.numel() not in (1, conv.out_channels):
        raise _err("%s: %s.weight_quantizer carries %d scales for %d output channels" % (who, nm, wq.scale.numel(), conv.out_channels))
    if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
        raise _err("%s: %s: padding mode not covered by the int8 blocks" % (who, nm))
    return wq


def _walk_iao8(model, input_hw=(32, 32), byte_ends=False, zero_points=False):
    """The graph walk of ``iao_compile_int8`` (no GPU needed): (first, layers, last, tail, flatten, report, pack_shuffle, ends); ``ends``: None, or with ``byte_ends``
    the layer dicts (first, last) of the two end blocks.  ``zero_points``: asymmetric quantizers are admitted; a layer whose input, weight, pool or consumer quantizer
    is asymmetric carries ``zp`` = True and takes the kernels of csrc/qgemm_iao8_zp.h."""
    if zero_points and byte_ends:
        raise _err("iao_compile_int8(zero_points=True): byte_ends=True is not covered together with zero points (the int8 end kernels take symmetric quantizers only)")
    from micronet_amd import _lib
    from micronet_amd.quantization.wqaq.dorefa.quantize import _is_ref_block
    from micronet_amd.quantization.wqaq.iao import quantize
    seq, prefix, flatten = _net_sequence(model, "iao_compile_int8")
    items = [(prefix + n_, c_) for n_, c_ in seq.named_children()]
    blocks = [i for i, (_, c_) in enumerate(items) if isinstance(getattr(c_, "conv", None), nn.Conv2d)]
    if len(blocks) < 3 or blocks[0] != 0:
        raise _err("iao_compile_int8: module order not recognised (expected a first conv block, at least one hidden block and a last conv block)")
    last_i = blocks[-1]
    (nm_first, first), (nm_last, last) = items[0], items[last_i]
    tail = [c_ for _, c_ in items[last_i + 1:]]

    ends_who = "iao_compile_int8(byte_ends=True)"

    def block_conv(nm, child, who="iao_compile_int8"):
        conv, bn, act = getattr(child, "conv", None), getattr(child, "bn", None), getattr(child, "relu", None)
        if not (_is_ref_block(child) and isinstance(bn, nn.Identity) and type(act) in (nn.ReLU, quantize.ReLUAfterFusedConv)):
            raise _err("%s: %s (%s): module order not recognised (expected a BN-folded conv -> Identity -> ReLU block)" % (who, nm, type(child).__name__))
        _iao8_check_conv(conv, nm + ".conv", who, zero_points)
        return conv

    if not isinstance(getattr(first, "conv", None), nn.Conv2d):
        raise _err("iao_compile_int8: %s: the first block holds no conv" % nm_first)
    last_conv = block_conv(nm_last, last)
    c0 = first.conv
    if byte_ends:
        block_conv(nm_first, first, ends_who)          # the first block is an int8 block too: the image goes through its own activation quantizer
        _iao8_check_weights(c0, nm_first + ".conv", ends_who)
        _iao8_check_weights(last_conv, nm_last + ".conv", ends_who)
    H, W = (_out_size(input_hw[i], c0.kernel_size[i], c0.stride[i], c0.padding[i], c0.dilation[i]) for i in (0, 1))
    layers, pack_shuffle = [], 0
    for nm, child in items[1:last_i]:
        if isinstance(child, nn.MaxPool2d):
            ok = (type(child) is quantize.QuantMaxPool2d and _pool_kind(child) == (2, 2, 0))
            if not ok:
                raise _err("iao_compile_int8: %s (%s, kernel %s, stride %s, padding %s): only a 2x2 / stride 2 QuantMaxPool2d is folded into the int8 block in front of it"
                           % (nm, type(child).__name__, child.kernel_size, child.stride, child.padding))
            if not layers and byte_ends:
                raise _err("%s: %s: a max-pool directly behind the first block is not covered (the pooled form of k_i8first is not built)" % (ends_who, nm))
            if not layers:
                raise _err("iao_compile_int8: %s: a max-pool directly behind the first block is not covered (its producer is not an int8 block)" % nm)
            if layers[-1]["pool"]:
                raise _err("iao_compile_int8: %s: a second max-pool behind one block" % nm)
            _iao8_check_quantizer(child.activation_quantizer, nm + ".activation_quantizer", True, zero_points=zero_points)
            layers[-1]["pool"], layers[-1]["pool_module"], layers[-1]["pool_name"] = 1, child, nm
            continue
        conv = block_conv(nm, child)
        wq = _iao8_check_weights(conv, nm + ".conv", zero_points=zero_points)
        if not _lib.get_lib().mn_i8conv_supported(C.byref(_conv_geom(conv)), conv.activation_quantizer.bits, wq.bits):
            raise _err("iao_compile_int8: %s.conv: geometry not covered by mn_i8conv_supported (%dx%d, stride %d, padding %d, dilation %d, groups %d, %d channels per group: "
                       "1x1 / padding 0 with groups 1 or C / groups %% 16 == 0, or 3x3 / padding 1 with C / groups %% 16 == 0; stride 1)"
                       % (nm, conv.kernel_size[0], conv.kernel_size[1], _one(conv.stride), _one(conv.padding), _one(conv.dilation), conv.groups, conv.in_channels // conv.groups))
        s = _shuffle_in_front("iao_compile_int8", nm, child, conv)
        if s:
            _check_shuffle_divides("iao_compile_int8", nm, conv, s)
            if layers:
                layers[-1]["shuffle"] = s          # folded into the producer's destination positions
            else:
                pack_shuffle = s                   # ... or into the pack behind the first block
        layers.append(dict(name=nm, conv=conv, k=conv.kernel_size[0], pad=conv.padding[0], cin=conv.in_channels, cout=conv.out_channels, groups=conv.groups, pool=0,
                           pool_module=None, pool_name=None, shuffle=0, w_bits=wq.bits, in_bits=conv.activation_quantizer.bits, per_channel=wq.scale.numel() > 1))
    if not layers:
        raise _err("iao_compile_int8: no hidden block between %s and %s" % (nm_first, nm_last))
    # the consumer of every hidden block: the next hidden conv's activation quantizer, or the last conv's
    is_asym = lambda q: int(zero_points and q._q_type_static == 1)
    for L, nxt in zip(layers, [M["conv"] for M in layers[1:]] + [last_conv]):
        L["consumer"] = nxt.activation_quantizer
        L["a_bits"] = nxt.activation_quantizer.bits
        L["asym_a"], L["asym_w"] = is_asym(L["conv"].activation_quantizer), is_asym(L["conv"].weight_quantizer)
        L["asym_out"] = is_asym(nxt.activation_quantizer)
        L["asym_p"] = is_asym(L["pool_module"].activation_quantizer) if L["pool"] else L["asym_out"]
        L["zp"] = bool(L["asym_a"] or L["asym_w"] or L["asym_out"] or L["asym_p"])
        if L["pool"] and L["pool_module"].activation_quantizer.bits != L["a_bits"]:
            raise _err("iao_compile_int8: %s: the pool's quantizer has %d bits, its consumer %d: one code width per block"
                       % (L["pool_name"], L["pool_module"].activation_quantizer.bits, L["a_bits"]))
    report = [dict(name=nm_first, kind="first", kernel="the model's own block (fp32), %s" % ("k_i8z_pack" if layers[0]["asym_a"] else "k_i8_pack"),
                   k=c0.kernel_size[0], cin=c0.in_channels, cout=c0.out_channels, groups=c0.groups, pool=0, out_order=("shuffle %d" % pack_shuffle) if pack_shuffle else "identity", table_bytes=0,
                   act_bytes_in=4 * c0.in_channels * input_hw[0] * input_hw[1], act_bytes_out=4 * c0.out_channels * H * W + _blocked(c0.out_channels, H, W))]
    ends = None
    if byte_ends:
        # the first block: an int8 block whose input is the fp32 image (mn_i8first_*), its consumer the first hidden conv's activation quantizer
        bits = (c0.activation_quantizer.bits, layers[0]["in_bits"], c0.weight_quantizer.bits)
        g = _conv_geom(c0, 1, input_hw[0], input_hw[1], _shuffle_in_front(ends_who, nm_first, first, c0))
        if not _lib.get_lib().mn_i8first_supported(C.byref(g), *bits):
            raise _err("%s: %s.conv: geometry not covered by mn_i8first_supported (%dx%d, stride %s, padding %s, dilation %s, groups %d, %d input channels, in_shuffle %d, "
                       "a %d x %d image: groups 1, no channel shuffle, 3x3 or 5x5 / stride 1 / dilation 1 / padding (KS - 1) / 2, C * KS * KS <= 128 and an LDS tile "
                       "C * (min(H, 255 / W + 2) + KS - 1) * (W + KS - 1) <= 32768: every W <= 512)"
                       % (ends_who, nm_first, c0.kernel_size[0], c0.kernel_size[1], c0.stride, c0.padding, c0.dilation, c0.groups, c0.in_channels, g.in_shuffle,
                          input_hw[0], input_hw[1]))
        Lf = dict(name=nm_first, conv=c0, k=c0.kernel_size[0], pad=c0.padding[0], cin=c0.in_channels, cout=c0.out_channels, groups=1, pool=0, shuffle=pack_shuffle,
                  in_bits=bits[0], a_bits=bits[1], w_bits=bits[2], per_channel=c0.weight_quantizer.scale.numel() > 1, consumer=layers[0]["conv"].activation_quantizer,
                  table_bytes=int(_lib.get_lib().mn_i8first_table_bytes(C.byref(g), *bits)))
        report[0] = dict(report[0], kind="int8_first", kernel="k_i8first<%d>" % Lf["k"], table_bytes=Lf["table_bytes"], act_bytes_out=_blocked(Lf["cout"], H, W))
    for L in layers:
        g = _block_geom(L)
        nin = _blocked(L["cin"], H, W)
        if L["pool"]:
            if H % 2 or W % 2:
                raise _err("iao_compile_int8: %s: the 2x2 max-pool behind it does not fit a %d x %d map" % (L["name"], H, W))
            H, W = H // 2, W // 2
        table_bytes = _lib.get_lib().mn_i8zconv_table_bytes if L["zp"] else _lib.get_lib().mn_i8conv_table_bytes
        L["table_bytes"] = int(table_bytes(C.byref(g), L["a_bits"], L["w_bits"]))
        report.append(dict(name=L["name"], kind="int8", kernel=_i8conv_kernel_name(L["k"], L["pool"], L["zp"]), k=L["k"], cin=L["cin"],
                           cout=L["cout"], groups=L["groups"], pool=L["pool"], out_order=("shuffle %d" % L["shuffle"]) if L["shuffle"] else "identity", table_bytes=L["table_bytes"], act_bytes_in=nin,
                           act_bytes_out=_blocked(L["cout"], H, W)))
    report.append(dict(name=nm_last, kind="last", kernel="%s, the model's own block (fp32)" % ("k_i8z_unpack" if layers[-1]["asym_out"] else "k_i8_unpack"),
                       k=last_conv.kernel_size[0], cin=last_conv.in_channels, cout=last_conv.out_channels, groups=last_conv.groups, pool=0, out_order="identity", table_bytes=0,
                       act_bytes_in=_blocked(last_conv.in_channels, H, W) + 4 * last_conv.in_channels * H * W, act_bytes_out=4 * last_conv.out_channels * H * W))
    if byte_ends:
        # the last block: the hidden kernel's contraction, stopped at r and written as the fp32 map of the tail (mn_i8conv_fwd_f32)
        bits = (last_conv.activation_quantizer.bits, last_conv.weight_quantizer.bits)
        if _shuffle_in_front(ends_who, nm_last, last, last_conv):
            raise _err("%s: %s: a channel shuffle in front of the last block is not covered (folding it into the last hidden block is not built)" % (ends_who, nm_last))
        g = _conv_geom(last_conv)
        if not _lib.get_lib().mn_i8conv_supported(C.byref(g), *bits):
            raise _err("%s: %s.conv: geometry not covered by mn_i8conv_supported, the rule of mn_i8conv_fwd_f32 (%dx%d, stride %s, padding %s, dilation %s, groups %d, "
                       "%d channels per group: 1x1 / padding 0 with groups 1 or C / groups %% 16 == 0, or 3x3 / padding 1 with C / groups %% 16 == 0; stride 1)"
                       % (ends_who, nm_last, last_conv.kernel_size[0], last_conv.kernel_size[1], last_conv.stride, last_conv.padding, last_conv.dilation,
                          last_conv.groups, last_conv.in_channels // last_conv.groups))
        Ll = dict(name=nm_last, conv=last_conv, k=last_conv.kernel_size[0], pad=last_conv.padding[0], cin=last_conv.in_channels, cout=last_conv.out_channels,
                  groups=last_conv.groups, pool=0, shuffle=0, a_bits=bits[0], w_bits=bits[1], per_channel=last_conv.weight_quantizer.scale.numel() > 1, relu=1,
                  table_bytes=int(_lib.get_lib().mn_i8conv_table_bytes(C.byref(g), *bits)))
        report[-1] = dict(report[-1], kind="int8_last", kernel="k_i8conv_f32<%d>" % Ll["k"], table_bytes=Ll["table_bytes"], act_bytes_in=_blocked(Ll["cin"], H, W))
        ends = (Lf, Ll)
    return first, layers, last, tail, flatten, report, pack_shuffle, ends


def iao_int8_report(model, input_hw=(32, 32), byte_ends=False, zero_points=False, end_to_end=False):
    """The ``report`` ``iao_compile_int8(model, byte_ends)`` would carry -- one row per stage: layer, kernel, geometry, folded pool, the consumer's shuffle folded into
    the stage (``out_order``), table bytes and the activation bytes per image the stage reads and writes at an ``input_hw`` input -- from the graph walk alone: no GPU,
    nothing packed.  With ``byte_ends`` the two end rows are the kinds ``int8_first`` / ``int8_last`` and no fp32 map stands between the rows.  Raises like
    ``iao_compile_int8`` for whatever the int8 blocks do not cover (weights off the grid excepted: that is read from the packed tables).

    The reference ResNet tree takes the walk of ``_walk_iao8_res``: one row per conv -- kind ``int8`` (a conv stage) or ``int8_add`` (the last conv of a block with its
    QuantAdd), between ``first`` (conv1 and its packs) and ``last`` (the unpack, avg_pool, fc) -- with kernel, geometry, ``stride``, ``relu``, ``shortcut``, the number
    of output maps ``nout`` and their ``consumers``, table bytes and activation bytes in and out per image.

    ``zero_points=True``: the walk of ``iao_compile_int8(model, zero_points=True)``: a stage with an asymmetric quantizer reports ``k_i8zconv<KS,pool>``, and the two
    end rows name ``k_i8z_pack`` / ``k_i8z_unpack`` where their quantizer is asymmetric; a symmetric net reports as without it.

    ``end_to_end=True`` (the reference ResNet tree only): the walk of ``iao_compile_int8(model, end_to_end=True)``: row 0 is the kind ``int8_first`` on
    ``k_i8first2<KS,nout>``, the last row the kind ``int8_last`` on ``k_i8poolfc``, both with table bytes and activation bytes (fp32 image in, ``nout`` byte maps out;
    bytes in, 4 O out); every row between them is the default report's."""
    if _is_ref_resnet(model):
        if zero_points:
            raise _err(_ZP_RESNET)
        return _walk_iao8_res(model, input_hw, byte_ends, end_to_end)[4]
    report = _walk_iao8(model, input_hw, byte_ends, zero_points)[5]
    if end_to_end:
        raise _err(_E2E_RESNET)
    return report


_E2E_RESNET = "iao_compile_int8(end_to_end=True): covered for the reference ResNet tree only (nin_gc's form is byte_ends=True)"
_ZP_RESNET = ("iao_compile_int8(zero_points=True): the reference ResNet tree is not covered with zero points (its strided and QuantAdd stages take symmetric "
              "quantizers only)")


def _iao8_ends_image(ends, x, keyword):
    """The fp32 image a plan with int8 ends (``keyword``: byte_ends or end_to_end) takes, contiguous."""
    Lf = ends[0] if ends else None
    if not (Lf and type(x) is torch.Tensor and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == Lf["cin"]):
        raise _err("iao_compile_int8(%s=True): the input must be a float32 GPU image [N, %s, H, W] of %s %s plan (no CPU fallback)"
                   % (keyword, Lf["cin"] if Lf else "C", "an" if keyword[0] in "aeiou" else "a", keyword))
    return x.contiguous()


def _iao8_ends_codes(ends, codes, N, H, W, keyword):
    """The last end's dict and the blocked codes ``run_last`` takes, contiguous."""
    Ll = ends[1] if ends else None
    if not (Ll and _is_code_map(codes, N, Ll["cin"], H * W)):
        raise _err("iao_compile_int8(%s=True): run_last needs %s %s plan and int8 GPU codes [N, ceil(C / 16), H * W, 16]"
                   % (keyword, "an" if keyword[0] in "aeiou" else "a", keyword))
    return Ll, codes.contiguous()


def _two_outs(q, L, nout):
    """The fields ``I8ResAdd`` and ``I8FirstOuts`` share: the scale and width of each output map; one map: the second pair repeats the first."""
    i = 1 if nout == 2 else 0
    q.nout, q.s_out0, q.bits0, q.s_out1, q.bits1 = nout, L["s_out"][0], L["out_bits"][0], L["s_out"][i], L["out_bits"][i]
    return q


class Int8Plan(_Plan):
    """What ``iao_compile_int8`` returns: the model's own first block (fp32) -> ``mn_i8_pack_codes`` at the second conv's scale -> one ``mn_i8conv_fwd`` per hidden
    block (2x2 max-pool and the consumer's channel shuffle folded in) -> ``mn_i8_unpack_codes`` at the last conv's scale -> the model's own last block and tail (its
    quantizer reproduces the same codes: fl(fl(c s) / s) rounds back to c).  Eval only; owns the packed weight tables and one set of byte buffers per input shape.
    ``layers[i]`` keeps what the table was packed from (w, s_w, bias, s_a, s_p, s_out, a_bits, w_bits, pool, shuffle) for the tests' judge.

    A plan compiled with ``zero_points=True`` runs a stage with an asymmetric quantizer on ``mn_i8zconv_fwd`` (``layers[i]["zp"]``; bytes are code - h, see
    ``csrc/qgemm_iao8_zp.h``), packs with ``mn_i8z_pack_codes`` and unpacks with ``mn_i8z_unpack_codes`` where that end's quantizer is asymmetric (``pack["q"]``,
    ``pack["unpack_q"]``), and ``layers[i]`` additionally keeps the zero points ``z_a``, ``z_w`` (a tensor like ``s_w``), ``z_p``, ``z_out`` and the flags ``asym_a``,
    ``asym_w``, ``asym_p``, ``asym_out``.

    With ``byte_ends`` (``ends`` is set) neither end runs the model's own modules: ``mn_i8first_fwd`` takes the fp32 image to the first hidden block's codes, the hidden
    stages run unchanged, ``mn_i8conv_fwd_f32`` takes the last hidden codes to the fp32 map [N][O][H * W] of the model's tail: no ``k_i8_pack``, no ``k_i8_unpack``
    and no fp32 activation map in between.  ``ends`` = (first, last) keeps what the two tables were packed from, as ``layers[i]`` does (the first also ``in_bits``)."""

    who = "iao_compile_int8"

    def __init__(self, first, layers, last, tail, flatten, report, pack, ends=None):
        super().__init__(first, layers, last, tail, flatten, report)
        self.pack = pack                  # dict: s (the second conv's activation scale), a_bits, order
        self.ends = ends                  # None, or the layer dicts (first, last) of a byte_ends plan
        self.stage_codes = []

    def _plan_buffers(self, shape, device):
        """Byte buffers and the fp32 buffer in front of the last block (byte_ends: behind it) for one first-block output shape; byte_ends: the geometries of the two
        ends stand around the hidden ones."""
        N, Cc, H, W = shape
        if Cc != self.layers[0]["cin"]:
            raise _err("iao_compile_int8: %s produced %d channels, %s reads %d" % (self.report[0]["name"], Cc, self.layers[0]["name"], self.layers[0]["cin"]))
        bufs, geoms = [_code_map(N, Cc, H * W, device)], []
        if self.ends:
            geoms.append(_block_geom(self.ends[0], N, H, W))          # (stride 1, padding (k - 1) / 2: the image has the first block's H x W)
        for L in self.layers:
            geoms.append(_block_geom(L, N, H, W))
            if L["pool"]:
                if H % 2 or W % 2:
                    raise _err("iao_compile_int8: %s: the 2x2 max-pool behind it does not fit a %d x %d map" % (L["name"], H, W))
                H, W = H // 2, W // 2
            bufs.append(_code_map(N, L["cout"], H * W, device))
        if self.ends:
            geoms.append(_block_geom(self.ends[1], N, H, W))
        return (bufs, geoms, torch.empty((N, (self.ends[1] if self.ends else self.layers[-1])["cout"], H, W), dtype=torch.float32, device=device))

    def _first(self, g, x, out, st):
        """The first end (byte_ends): the fp32 image to the first hidden stage's codes."""
        from micronet_amd import ops
        Lf = self.ends[0]
        ops._call("mn_i8first_fwd", C.byref(g), Lf["in_bits"], Lf["a_bits"], Lf["w_bits"], ops._p(Lf["table"]), ops._p(x), ops._p(out), st)

    def _stage(self, L, g, src, out, st):
        """A hidden stage: the zero-point kernels where one of its quantizers is asymmetric."""
        from micronet_amd import ops
        ops._call("mn_i8zconv_fwd" if L.get("zp") else "mn_i8conv_fwd", C.byref(g), L["a_bits"], L["w_bits"], ops._p(L["table"]), ops._p(src), ops._p(out),
                  int(L["pool"]), st)

    def _last(self, g, codes, y, st):
        """The last end (byte_ends): the last hidden codes to the fp32 map of the tail."""
        from micronet_amd import ops
        Ll = self.ends[1]
        ops._call("mn_i8conv_fwd_f32", C.byref(g), Ll["a_bits"], Ll["w_bits"], ops._p(Ll["table"]), ops._p(codes), ops._p(y), Ll["relu"], st)

    def run_first(self, x):
        """The first block alone on the fp32 image (byte_ends): the blocked codes [N, ceil(cout / 16), H * W, 16] the first hidden stage reads, freshly allocated
        (tests)."""
        from micronet_amd import ops
        x = _iao8_ends_image(self.ends, x, "byte_ends")
        Lf, (N, _, H, W) = self.ends[0], x.shape
        out = _code_map(N, Lf["cout"], H * W, x.device, fill=77)
        with torch.cuda.device(x.device):
            self._first(_block_geom(Lf, N, H, W), x, out, ops._s())
        return out

    def run_last(self, codes, N, H, W):
        """The last block alone on blocked input codes [N, ceil(cin / 16), H * W, 16] (byte_ends): the fp32 map [N, cout, H, W] of the tail, freshly allocated (tests)."""
        from micronet_amd import ops
        Ll, codes = _iao8_ends_codes(self.ends, codes, N, H, W, "byte_ends")
        out = torch.full((N, Ll["cout"], H, W), float("nan"), dtype=torch.float32, device=codes.device)
        with torch.cuda.device(codes.device):
            self._last(_block_geom(Ll, N, H, W), codes, out, ops._s())
        return out

    def _forward_ends(self, x):
        from micronet_amd import ops
        x = _iao8_ends_image(self.ends, x, "byte_ends")
        N, _, H, W = x.shape
        with torch.cuda.device(x.device):
            bufs, geoms, y = self._shape_buffers((N, self.ends[0]["cout"], H, W), x.device)
            st = ops._s()
            self._first(geoms[0], x, bufs[0], st)
            for i, L in enumerate(self.layers):
                self._stage(L, geoms[i + 1], bufs[i], bufs[i + 1], st)
            if self.keep_stages:
                self.stage_codes = [b.clone() for b in bufs]
            self._last(geoms[-1], bufs[-1], y, st)
        return self._finish(y if len(self.tail) else y.clone())          # (the buffer belongs to the plan: never handed out)

    def run_stage(self, i, codes, N, H, W):
        """Hidden stage ``i`` alone on blocked input codes [N, ceil(cin / 16), H * W, 16] (int8, GPU): its blocked output codes, freshly allocated (tests)."""
        from micronet_amd import ops
        L = self.layers[i]
        if not _is_code_map(codes, N, L["cin"], H * W):
            raise _err("iao_compile_int8: run_stage needs int8 GPU codes [N, ceil(C / 16), H * W, 16]")
        Ho, Wo = (H // 2, W // 2) if L["pool"] else (H, W)
        out = _code_map(N, L["cout"], Ho * Wo, codes.device, fill=77)
        with torch.cuda.device(codes.device):
            self._stage(L, _block_geom(L, N, H, W), codes.contiguous(), out, ops._s())
        return out

    @torch.no_grad()
    def forward(self, x):
        from micronet_amd import ops
        if self.ends:
            return self._forward_ends(x)
        a = self.first(x)
        if not (type(a) is torch.Tensor and a.is_cuda and a.dtype == torch.float32 and a.dim() == 4):
            raise _err("iao_compile_int8: %s did not produce a float32 GPU map (the input must be a float32 GPU tensor; no CPU fallback)" % self.report[0]["name"])
        a = a.contiguous()
        N, Cc, H, W = a.shape
        with torch.cuda.device(a.device):
            bufs, geoms, y = self._shape_buffers(a.shape, a.device)
            st = ops._s()
            if self.pack.get("q") is not None:
                ops._call("mn_i8z_pack_codes", ops._p(a), N, Cc, H * W, C.byref(self.pack["q"]), ops._p(self.pack["order"]), ops._p(bufs[0]), st)
            else:
                ops._call("mn_i8_pack_codes", ops._p(a), N, Cc, H * W, self.pack["s"], self.pack["a_bits"], ops._p(self.pack["order"]), ops._p(bufs[0]), st)
            for i, L in enumerate(self.layers):
                self._stage(L, geoms[i], bufs[i], bufs[i + 1], st)
            if self.keep_stages:
                self.stage_codes = [b.clone() for b in bufs]
            n_, c_, h_, w_ = y.shape
            if self.pack.get("unpack_q") is not None:
                ops._call("mn_i8z_unpack_codes", ops._p(bufs[-1]), n_, c_, h_ * w_, C.byref(self.pack["unpack_q"]), ops._p(y), st)
            else:
                ops._call("mn_i8_unpack_codes", ops._p(bufs[-1]), n_, c_, h_ * w_, self.layers[-1]["s_out"], ops._p(y), st)
        return self._finish(self.last(y))


def _iao8_constants(qs):
    """{id(q): (scale, zero point)} of the per-tensor quantizers ``qs``, in ONE host read (compile time: the one place a host read-back is allowed)."""
    vals = torch.cat([t.detach().float().reshape(-1)[:1] for q in qs for t in (q.scale, q.zero_point)]).tolist()
    return {id(q): (vals[2 * i], vals[2 * i + 1]) for i, q in enumerate(qs)}


def _iao8_packed_from(L, m, dev):
    """The fields of a layer's dict its table is packed from, and the empty table: ``m`` is the conv, or the fc."""
    L["w"] = m.weight.detach().float().contiguous()
    L["s_w"] = m.weight_quantizer.scale.detach().float().reshape(-1).contiguous()
    L["bias"] = m.bias.detach().float().contiguous() if m.bias is not None else None
    L["table"] = torch.empty(L["table_bytes"] // 4, dtype=torch.int32, device=dev)


def _iao8_counters(packed):
    """The counters of every packed table, in one host read: header words 0 and 7, and 13 .. 15, which count in the zero-point tables alone (the other tables keep
    what they like there: ``_iao8_check_counters`` reads them under ``zp`` only)."""
    return torch.stack([L["table"][[0, 7, 13, 14, 15]] for L in packed]).tolist()


def _iao8_check_counters(who, nm, L, row, scales, zp=False):
    """Refuse a table whose counters ``row`` are not all 0; ``nm``: the displayed name, ``scales``: the activation scales the table was packed with, ``zp``: a
    zero-point table."""
    bad, off, zbad, wide, nopad = row
    if bad:
        raise _err("%s: %s: %d rows or scales with a non-finite or non-positive constant (al, bias, s_w, %s)" % (who, nm, bad, scales))
    if zp and zbad:
        raise _err("%s: %s: %d zero points (of the input, pool and consumer quantizers and the rows' z_w) that are not integers of magnitude <= 65535" % (who, nm, zbad))
    if off:
        raise _err("%s: %s: %d rows whose stored weights are off the grid k * s_w (run prequantize_weights after iao_model_bn_fuse)" % (who, nm, off))
    if zp and wide:
        raise _err("%s: %s: %d rows whose sum over %d channels x %d taps does not fit int32 at these zero points" % (who, nm, wide, L["cin"] // L["groups"], L["k"] * L["k"]))
    if zp and nopad:
        raise _err("%s: %s: zero padding has no byte: the value 0 is not a code of the input quantizer (zero point %g) of this 3x3 stage" % (who, nm, L["z_a"]))


@torch.no_grad()
def iao_compile_int8(model, byte_ends=False, zero_points=False, end_to_end=False):
    """``model``: the result of ``iao_model_bn_fuse`` + ``prequantize_weights`` on a symmetric IAO net, on the GPU (the reference's ``nin_gc``, or an ``nn.Sequential``
    of its block kinds).  Returns an ``Int8Plan`` that keeps every hidden activation as one int8 code and contracts on v_mfma_i32_16x16x64_i8
    (``csrc/qgemm_iao8.h``); the two ends stay on the model's own modules.  ``.report`` lists the stages.  Scales are read from the quantizer buffers and the table
    counters read back here, once.  Anything the int8 blocks do not cover -- an asymmetric or 32-bit quantizer, a per-tensor scale that is not a single value, a layer
    that is not ``quant_inference``, weights off the grid, a geometry ``mn_i8conv_supported`` refuses, a pool other than a 2x2 / 2 ``QuantMaxPool2d``, a pool directly
    behind the first block -- raises ``MicronetHipError`` naming the layer: never a silent fp32 path (the caller still has ``model``).

    ``byte_ends=True``: the two ends run on the int8 kernels as well (``csrc/qgemm_iao8_ends.h``): the first conv quantises the fp32 image with its own activation
    quantizer on the way in and writes the first hidden block's codes, the last conv writes the fp32 map of the model's tail (``QuantAvgPool2d``, ...) straight from
    the last hidden codes.  The first block must be a BN-folded ``quant_inference`` block like the hidden ones with a geometry ``mn_i8first_supported`` covers (3x3 or
    5x5, C * KS * KS <= 128, no pool behind it), the last one a geometry ``mn_i8conv_supported`` covers; anything else raises naming the layer.

    The reference ResNet tree (BasicBlock and BottleNeck nets, ``bn_fuse=True``, folded and pre-quantised) returns an ``Int8ResPlan``: strided convs, shortcut convs
    and the QuantAdd run on byte codes (``csrc/qgemm_iao8_res.h``), every block output is written once per consumer quantizer, and conv1, avg_pool and fc stay on the
    model's own modules.  ``byte_ends=True`` raises for it.

    ``end_to_end=True`` (the reference ResNet tree only; every other model raises, nin_gc's form being ``byte_ends=True``): the two ends of the ``Int8ResPlan`` run
    on bytes as well (``csrc/qgemm_iao8_e2e.h``).  ``mn_i8first_fwd2`` takes the fp32 image through conv1 to one code map per consumer quantizer, the stages run
    unchanged, ``mn_i8poolfc_fwd`` takes the last block's codes through avg_pool and fc to the fp32 logits: no fp32 activation map, no pack, no unpack.  conv1 must
    be a BN-folded ``quant_inference`` ``QuantConv2d`` with ReLU, a symmetric single-scale activation quantizer and a geometry ``mn_i8first_supported`` covers (3x3
    or 5x5, stride 1), avg_pool a ``QuantAdaptiveAvgPool2d`` to 1 x 1, fc a ``quant_inference`` ``QuantLinear`` (set ``model.fc.quant_inference = True`` before
    ``prequantize_weights``: ``iao_model_bn_fuse`` marks the convs only) with symmetric quantizers that ``mn_i8poolfc_supported`` covers (at most 64 outputs); every refusal raises ``iao_compile_int8(end_to_end=True): <layer>: <rule>``.  Together with ``byte_ends``
    or ``zero_points`` the message of that keyword wins.

    ``zero_points=True``: a net prepared with ``q_type=1`` compiles as well.  Asymmetric quantizers (``AsymmetricQuantizer``, 2 .. 8 bits, an activation quantizer with
    a single zero point, a weight quantizer with as many zero points as scales) are admitted; a hidden stage any of whose four quantizers -- input activation, weight,
    pool, consumer -- is asymmetric runs on ``mn_i8zconv_fwd`` (``csrc/qgemm_iao8_zp.h``: bytes are code - h, the zero points enter as integer offsets of an exact
    int32 sum), every other stage on ``mn_i8conv_fwd`` as before, and a symmetric net gives the plan and report it gives without the keyword.  The table counters
    additionally refuse, naming the layer: a zero point that is not an integer of magnitude <= 65535, a sum that would not fit int32, and a 3x3 stage whose input
    quantizer has no code for the value 0 ("zero padding has no byte").  Not covered, each raising: together with ``byte_ends=True``; the reference ResNet tree."""
    from micronet_amd import _lib, ops
    if _is_ref_resnet(model):
        if zero_points:
            raise _err(_ZP_RESNET)
        return _compile_iao8_res(model, byte_ends, end_to_end)
    who = "iao_compile_int8(byte_ends=True)" if byte_ends else "iao_compile_int8"
    first, layers, last, tail, flatten, report, pack_shuffle, ends = _walk_iao8(model, byte_ends=byte_ends, zero_points=zero_points)
    if end_to_end:
        raise _err(_E2E_RESNET)
    _require_gpu(model, "iao_compile_int8")
    dev = layers[0]["conv"].weight.device
    packed = ([ends[0]] if ends else []) + layers + ([ends[1]] if ends else [])
    const = _iao8_constants([q for L in packed for q in (L["conv"].activation_quantizer, L.get("consumer"), getattr(L.get("pool_module"), "activation_quantizer", None))
                             if q is not None])

    def packed_from(L, conv):
        _iao8_packed_from(L, conv, dev)
        L["s_a"], L["z_a"] = const[id(conv.activation_quantizer)]
        L["z_w"] = conv.weight_quantizer.zero_point.detach().float().reshape(-1).contiguous()
        L["out_order"] = _shuffle_order(L["cout"], L["shuffle"], dev) if L["shuffle"] else None

    with torch.cuda.device(dev):
        if ends:
            Lf, Ll = ends
            packed_from(Lf, Lf.pop("conv"))
            Lf["s_out"] = const[id(Lf.pop("consumer"))][0]
            ops._call("mn_i8first_pack", C.byref(_block_geom(Lf)), ops._p(Lf["w"]), ops._p(Lf["s_w"]), 1 if Lf["per_channel"] else 0, ops._p(Lf["bias"]), Lf["s_a"],
                      Lf["s_out"], Lf["in_bits"], Lf["a_bits"], Lf["w_bits"], ops._p(Lf["out_order"]), ops._p(Lf["table"]), ops._s())
            packed_from(Ll, Ll.pop("conv"))
            Ll["s_p"] = Ll["s_out"] = 1.0          # (mn_i8conv_fwd_f32 stops at r: neither is read)
            ops._call("mn_i8conv_pack", C.byref(_block_geom(Ll)), ops._p(Ll["w"]), ops._p(Ll["s_w"]), 1 if Ll["per_channel"] else 0, ops._p(Ll["bias"]), Ll["s_a"], 1.0, 1.0,
                      Ll["a_bits"], Ll["w_bits"], None, ops._p(Ll["table"]), ops._s())
        for L in layers:
            conv, pool_m = L.pop("conv"), L.pop("pool_module")
            packed_from(L, conv)
            L["s_out"], L["z_out"] = const[id(L.pop("consumer"))]
            L["s_p"], L["z_p"] = const[id(pool_m.activation_quantizer)] if pool_m is not None else (L["s_out"], L["z_out"])
            if L["zp"]:
                qa, qp, qo = (_lib.I8ZQuant(L["s_a"], L["z_a"], L["asym_a"], L["in_bits"]), _lib.I8ZQuant(L["s_p"], L["z_p"], L["asym_p"], L["a_bits"]),
                              _lib.I8ZQuant(L["s_out"], L["z_out"], L["asym_out"], L["a_bits"]))
                ops._call("mn_i8zconv_pack", C.byref(_block_geom(L)), ops._p(L["w"]), ops._p(L["s_w"]), ops._p(L["z_w"]), 1 if L["per_channel"] else 0, ops._p(L["bias"]),
                          C.byref(qa), C.byref(qp), C.byref(qo), L["asym_w"], L["w_bits"], ops._p(L["out_order"]), ops._p(L["table"]), ops._s())
            else:
                ops._call("mn_i8conv_pack", C.byref(_block_geom(L)), ops._p(L["w"]), ops._p(L["s_w"]), 1 if L["per_channel"] else 0, ops._p(L["bias"]), L["s_a"], L["s_p"],
                          L["s_out"], L["a_bits"], L["w_bits"], ops._p(L["out_order"]), ops._p(L["table"]), ops._s())
        counters = _iao8_counters(packed)
    for L, row in zip(packed, counters):
        _iao8_check_counters(who, L["name"] + ".conv", L, row, "s_a, s_p, s_out", zp=L.get("zp"))
    pack = dict(s=layers[0]["s_a"], a_bits=layers[0]["in_bits"], order=_shuffle_order(layers[0]["cin"], pack_shuffle, dev) if pack_shuffle else None)
    if layers[0].get("asym_a"):
        pack["q"] = _lib.I8ZQuant(layers[0]["s_a"], layers[0]["z_a"], 1, layers[0]["in_bits"])
    if layers[-1].get("asym_out"):
        pack["unpack_q"] = _lib.I8ZQuant(layers[-1]["s_out"], layers[-1]["z_out"], 1, layers[-1]["a_bits"])
    return Int8Plan(first, layers, last, tail, flatten, report, pack, ends)


# ------------------------------------------------------------------------------------------------ int8 deployment of BN-folded IAO ResNets (csrc/qgemm_iao8_res.h)
_RESNET_STAGES = ("conv2_x", "conv3_x", "conv4_x", "conv5_x")


def _is_ref_resnet(model):
    """The reference ResNet tree: conv1, conv2_x .. conv5_x of blocks with residual_function / shortcut / add, avg_pool, fc."""
    if not all(isinstance(getattr(model, n_, None), nn.Sequential) for n_ in ("conv1",) + _RESNET_STAGES) or not hasattr(model, "avg_pool") or not hasattr(model, "fc"):
        return False
    return all(hasattr(b_, "residual_function") and hasattr(b_, "shortcut") and hasattr(b_, "add") for n_ in _RESNET_STAGES for b_ in getattr(model, n_))


def _walk_iao8_res(model, input_hw=(32, 32), byte_ends=False, end_to_end=False):
    """The graph walk of ``iao_compile_int8`` on the reference ResNet tree (no GPU needed): (stem, stages, buffers, tail quantizer, report).  ``end_to_end``: conv1,
    avg_pool and fc are held to the rules of the byte ends (csrc/qgemm_iao8_e2e.h), ``stem["ends"]`` = (first, last) are their layer dicts and the two end rows of the
    report are the kinds ``int8_first`` / ``int8_last``.

    A VALUE -- conv1's output, or a block's output v = relu(add) -- has up to two consumers with a quantizer each: the next block's first conv, and the next block's
    shortcut (its QuantAdd itself for an identity shortcut, else the shortcut conv's activation quantizer).  Its producer writes one code map per consumer quantizer
    (``outs``); ``buffers[i]`` is the channel count of code map i.  The last block writes one map at avg_pool's activation quantizer."""
    from micronet_amd import _lib
    from micronet_amd.quantization.wqaq.iao import quantize
    who = "iao_compile_int8"
    if byte_ends:
        raise _err("iao_compile_int8(byte_ends=True): conv1: a ResNet's first conv feeds two consumers with a quantizer each (the first block's conv and its shortcut); "
                   "the two-output form of k_i8first is not built")

    def conv_chain(nm, seq):
        """[(name, conv, relu)] of a Sequential of BN-folded conv -> Identity [-> ReLU] groups."""
        kids, out, i = list(seq.named_children()), [], 0
        while i < len(kids):
            n_, c_ = kids[i]
            if not isinstance(c_, nn.Conv2d) or i + 1 >= len(kids) or not isinstance(kids[i + 1][1], nn.Identity):
                raise _err("%s: %s.%s (%s): module order not recognised (expected BN-folded conv -> Identity [-> ReLU] groups; run iao_model_bn_fuse on a bn_fuse=True net)"
                           % (who, nm, n_, type(c_).__name__))
            relu = i + 2 < len(kids) and isinstance(kids[i + 2][1], nn.ReLU)
            out.append((nm + "." + n_, c_, relu))
            i += 3 if relu else 2
        return out

    def check_conv(nm, conv):
        _iao8_check_conv(conv, nm, who)
        return _iao8_check_weights(conv, nm, who)

    stem_chain = conv_chain("conv1", model.conv1)
    if len(stem_chain) != 1 or not stem_chain[0][2]:
        raise _err("%s: conv1: module order not recognised (expected one BN-folded conv -> Identity -> ReLU)" % who)
    c0 = stem_chain[0][1]
    _iao8_check_conv(c0, "conv1.0", who, fold_only=True)          # (all the default plan asks of conv1: it runs on the model's own module)
    buffers = []

    def new_map(producer, q, qname, channels):
        buffers.append(channels)
        producer["outs"].append(dict(q=q, consumer=qname, buf=len(buffers) - 1))
        return len(buffers) - 1

    def new_stage(nm, conv, relu, kind, src, sc=None, shortcut=None):
        wq = check_conv(nm, conv)
        st = dict(name=nm, kind=kind, conv=conv, k=_one(conv.kernel_size), pad=_one(conv.padding), stride=_one(conv.stride), cin=conv.in_channels, cout=conv.out_channels,
                  groups=conv.groups, relu=int(relu), in_bits=conv.activation_quantizer.bits, w_bits=wq.bits, per_channel=wq.scale.numel() > 1, src=src, sc=sc,
                  shortcut=shortcut, outs=[])
        stages.append(st)
        return st

    stem = dict(name="conv1", cout=c0.out_channels, outs=[])
    stages, cur = [], stem          # cur: the producer of the current block's input value
    for sname in _RESNET_STAGES:
        for bname, blk in getattr(model, sname).named_children():
            nm = "%s.%s" % (sname, bname)
            add = blk.add
            if not isinstance(add, quantize.QuantAdd):
                raise _err("%s: %s.add (%s) is not an IAO QuantAdd (prepare() quantises the residual add)" % (who, nm, type(add).__name__))
            qadd = add.activation_quantizer
            _iao8_check_quantizer(qadd, nm + ".add.activation_quantizer", True, who)
            res, sc = conv_chain(nm + ".residual_function", blk.residual_function), conv_chain(nm + ".shortcut", blk.shortcut)
            if len(res) < 2 or not all(r_ for _, _, r_ in res[:-1]) or res[-1][2] or len(sc) > 1 or (sc and sc[0][2]):
                raise _err("%s: %s: module order not recognised (expected residual_function = conv -> Identity -> ReLU ... conv -> Identity and shortcut = empty or "
                           "conv -> Identity)" % (who, nm))
            cin = cur["cout"]
            if res[0][1].in_channels != cin or (sc and sc[0][1].in_channels != cin):
                raise _err("%s: %s reads %d channels, its producer %s writes %d" % (who, nm, res[0][1].in_channels, cur["name"], cin))
            map_a = new_map(cur, res[0][1].activation_quantizer, res[0][0] + ".activation_quantizer", cin)
            if sc:
                map_b = new_map(cur, sc[0][1].activation_quantizer, sc[0][0] + ".activation_quantizer", cin)
            else:
                map_b = new_map(cur, qadd, nm + ".add.activation_quantizer", cin)          # the identity shortcut: already a code of the block's QuantAdd
            src = map_a
            for (cn, conv, _), (nn_, nxt, _) in zip(res[:-1], res[1:]):
                st = new_stage(cn, conv, True, "int8", src)
                src = new_map(st, nxt.activation_quantizer, nn_ + ".activation_quantizer", conv.out_channels)
            if sc:
                st = new_stage(sc[0][0], sc[0][1], False, "int8", map_b)
                map_b = new_map(st, qadd, nm + ".add.activation_quantizer", sc[0][1].out_channels)
            cur = new_stage(res[-1][0], res[-1][1], False, "int8_add", src, sc=map_b, shortcut="conv" if sc else "identity")
            cur["add"], cur["add_name"] = qadd, nm + ".add"
            if buffers[map_b] != cur["cout"]:
                raise _err("%s: %s.add: the residual has %d channels, the shortcut %d" % (who, nm, cur["cout"], buffers[map_b]))
    if not stages:
        raise _err("%s: no residual block between conv1 and avg_pool" % who)
    tail_q = getattr(model.avg_pool, "activation_quantizer", None)
    _iao8_check_quantizer(tail_q, "avg_pool.activation_quantizer", True, who)
    new_map(cur, tail_q, "avg_pool.activation_quantizer", cur["cout"])

    # kernels, geometry rules and the report: one row per stage
    lib = _lib.get_lib()
    H0, W0 = (_out_size(input_hw[i], c0.kernel_size[i], c0.stride[i], c0.padding[i], c0.dilation[i]) for i in (0, 1))
    dims = {o["buf"]: (H0, W0) for o in stem["outs"]}
    report = [dict(name="conv1", kind="first", kernel="the model's own block (fp32), k_i8_pack x %d" % len(stem["outs"]), k=c0.kernel_size[0], cin=c0.in_channels,
                   cout=c0.out_channels, stride=c0.stride[0], relu=1, shortcut=None, nout=len(stem["outs"]), consumers=[o["consumer"] for o in stem["outs"]], table_bytes=0,
                   act_bytes_in=4 * c0.in_channels * input_hw[0] * input_hw[1], act_bytes_out=4 * c0.out_channels * H0 * W0 + len(stem["outs"]) * _blocked(c0.out_channels, H0, W0))]
    for st in stages:
        conv = st["conv"]
        st["out_bits"] = [o["q"].bits for o in st["outs"]]
        st["a_bits"] = st["add"].bits if st["kind"] == "int8_add" else st["out_bits"][0]          # the width of the codes the conv's epilogue forms
        g = _conv_geom(conv)
        what = ("%dx%d, stride %s, padding %s, dilation %s, groups %d, %d input channels" % (conv.kernel_size[0], conv.kernel_size[1], conv.stride, conv.padding,
                                                                                            conv.dilation, conv.groups, conv.in_channels))
        if st["kind"] == "int8" and st["relu"] and st["stride"] == 1 and st["in_bits"] == st["a_bits"]:
            st["api"] = "i8conv"          # the stride-1 ReLU convs keep running on the hidden blocks' kernel
            if not lib.mn_i8conv_supported(C.byref(g), st["a_bits"], st["w_bits"]):
                raise _err("%s: %s: geometry not covered by mn_i8conv_supported (%s: 1x1 / padding 0 with groups 1 or C / groups %% 16 == 0, or 3x3 / padding 1 with "
                           "C / groups %% 16 == 0; stride 1)" % (who, st["name"], what))
            st["table_bytes"] = int(lib.mn_i8conv_table_bytes(C.byref(g), st["a_bits"], st["w_bits"]))
            kernel = _i8conv_kernel_name(st["k"], 0)
        else:
            st["api"] = "res_add" if st["kind"] == "int8_add" else "res_conv"
            if not lib.mn_i8res_supported(C.byref(g), st["in_bits"], st["a_bits"], st["w_bits"]) or (st["api"] == "res_add" and st["stride"] != 1):
                raise _err("%s: %s: geometry not covered by mn_i8res_supported (%s: groups 1, dilation 1, 1x1 / padding 0 with any C or 3x3 / padding 1 with C %% 16 == 0, "
                           "stride 1 or 2 in both directions; the conv in front of a QuantAdd: stride 1)" % (who, st["name"], what))
            st["table_bytes"] = int(lib.mn_i8res_table_bytes(C.byref(g), st["in_bits"], st["a_bits"], st["w_bits"]))
            kernel = ("k_i8res_add<%d,%d>" % (st["k"], len(st["outs"]))) if st["api"] == "res_add" else "k_i8res_conv<%d,%d,%d>" % (st["k"], st["stride"], st["relu"])
        H, W = dims[st["src"]]
        Ho, Wo = (H - 1) // st["stride"] + 1, (W - 1) // st["stride"] + 1
        if st["sc"] is not None and dims[st["sc"]] != (Ho, Wo):
            raise _err("%s: %s: the residual map is %d x %d, the shortcut's %d x %d" % (who, st["add_name"], Ho, Wo, dims[st["sc"]][0], dims[st["sc"]][1]))
        for o in st["outs"]:
            dims[o["buf"]] = (Ho, Wo)
        report.append(dict(name=st["name"], kind=st["kind"], kernel=kernel, k=st["k"], cin=st["cin"], cout=st["cout"], stride=st["stride"], relu=st["relu"],
                           shortcut=st["shortcut"], nout=len(st["outs"]), consumers=[o["consumer"] for o in st["outs"]], table_bytes=st["table_bytes"],
                           act_bytes_in=_blocked(st["cin"], H, W) + (_blocked(st["cout"], Ho, Wo) if st["sc"] is not None else 0),
                           act_bytes_out=len(st["outs"]) * _blocked(st["cout"], Ho, Wo)))
    Hl, Wl = dims[cur["outs"][0]["buf"]]
    fc_out = getattr(model.fc, "out_features", 0)
    if end_to_end:
        who2 = "iao_compile_int8(end_to_end=True)"

        def held(layer, rule, *a):
            """``rule(*a)`` with its refusal re-raised as who2: <layer>: <rule>."""
            try:
                return rule(*a)
            except _lib.MicronetHipError as e:
                raise _err("%s: %s: %s" % (who2, layer, str(e).split(": ", 1)[-1]))
        wq0 = held("conv1.0", check_conv, "conv1.0", c0)
        Lf = dict(name="conv1.0", conv=c0, k=_one(c0.kernel_size), pad=_one(c0.padding), stride=_one(c0.stride), cin=c0.in_channels, cout=c0.out_channels,
                  in_bits=c0.activation_quantizer.bits, w_bits=wq0.bits, per_channel=wq0.scale.numel() > 1, outs=stem["outs"], out_bits=[o["q"].bits for o in stem["outs"]])
        g0 = _conv_geom(c0, 1, input_hw[0], input_hw[1])
        if not 1 <= len(stem["outs"]) <= 2 or not lib.mn_i8first_supported(C.byref(g0), Lf["in_bits"], Lf["out_bits"][0], Lf["w_bits"]):
            raise _err("%s: conv1.0: geometry not covered by mn_i8first_supported (%dx%d, stride %s, padding %s, dilation %s, groups %d, %d input channels: 3x3 or 5x5, "
                       "stride 1, dilation 1, padding (k - 1) / 2, groups 1, C * k * k <= 128)" % (who2, c0.kernel_size[0], c0.kernel_size[1], c0.stride, c0.padding,
                                                                                                     c0.dilation, c0.groups, c0.in_channels))
        Lf["table_bytes"] = int(lib.mn_i8first_table_bytes(C.byref(g0), Lf["in_bits"], Lf["out_bits"][0], Lf["w_bits"]))
        pool, fc = model.avg_pool, model.fc
        if not isinstance(pool, quantize.QuantAdaptiveAvgPool2d) or pool.output_size not in (1, (1, 1)):
            raise _err("%s: avg_pool: (%s) is not a QuantAdaptiveAvgPool2d to 1 x 1" % (who2, type(pool).__name__))
        if not isinstance(fc, quantize.QuantLinear):
            raise _err("%s: fc: (%s) is not an IAO QuantLinear" % (who2, type(fc).__name__))
        if not fc.quant_inference:
            raise _err("%s: fc: is not quant_inference: its stored weights are not on the grid (prequantize_weights)" % who2)
        held("fc", _iao8_check_quantizer, fc.activation_quantizer, "fc.activation_quantizer", True, who)
        held("fc", _iao8_check_quantizer, fc.weight_quantizer, "fc.weight_quantizer", False, who)
        if fc.weight_quantizer.scale.numel() not in (1, fc.out_features):
            raise _err("%s: fc: fc.weight_quantizer carries %d scales for %d outputs" % (who2, fc.weight_quantizer.scale.numel(), fc.out_features))
        if fc.in_features != cur["cout"]:
            raise _err("%s: fc: in_features is %d, the last block %s writes %d channels" % (who2, fc.in_features, cur["name"], cur["cout"]))
        Ll = dict(name="fc", fc=fc, cin=fc.in_features, cout=fc.out_features, p_bits=tail_q.bits, a_bits=fc.activation_quantizer.bits, w_bits=fc.weight_quantizer.bits,
                  per_channel=fc.weight_quantizer.scale.numel() > 1)
        if not lib.mn_i8poolfc_supported(1, Ll["cin"], Hl * Wl, Ll["cout"], Ll["p_bits"], Ll["a_bits"], Ll["w_bits"]):
            raise _err("%s: fc: shape not covered by mn_i8poolfc_supported (%d channels, a %d x %d map, %d outputs: 1 <= O <= 64, H * W <= 4096, "
                       "C * 2^(a-1) * (2^(w-1) - 1) <= INT_MAX)" % (who2, Ll["cin"], Hl, Wl, Ll["cout"]))
        Ll["table_bytes"] = int(lib.mn_i8poolfc_table_bytes(Ll["cin"], Ll["cout"], Ll["p_bits"], Ll["a_bits"], Ll["w_bits"]))
        stem["ends"] = (Lf, Ll)
        report[0] = dict(report[0], kind="int8_first", kernel="k_i8first2<%d,%d>" % (Lf["k"], len(stem["outs"])), table_bytes=Lf["table_bytes"],
                         act_bytes_out=len(stem["outs"]) * _blocked(c0.out_channels, H0, W0))
        report.append(dict(name="avg_pool", kind="int8_last", kernel="k_i8poolfc", k=0, cin=cur["cout"], cout=fc_out, stride=1, relu=0, shortcut=None, nout=1, consumers=[],
                           table_bytes=Ll["table_bytes"], act_bytes_in=_blocked(cur["cout"], Hl, Wl), act_bytes_out=4 * fc_out))
        return stem, stages, buffers, tail_q, report
    report.append(dict(name="avg_pool", kind="last", kernel="k_i8_unpack, the model's own avg_pool and fc (fp32)", k=0, cin=cur["cout"], cout=fc_out, stride=1, relu=0,
                       shortcut=None, nout=1, consumers=[], table_bytes=0, act_bytes_in=_blocked(cur["cout"], Hl, Wl) + 4 * cur["cout"] * Hl * Wl, act_bytes_out=4 * fc_out))
    return stem, stages, buffers, tail_q, report


class Int8ResPlan(_Plan):
    """What ``iao_compile_int8`` returns for a ResNet: the model's own conv1 (fp32) -> ``mn_i8_pack_codes`` once per consumer quantizer of its output -> one int8 kernel
    per conv (``mn_i8conv_fwd`` for the stride-1 ReLU convs, ``mn_i8res_conv_fwd`` for the strided ones and the shortcut convs, ``mn_i8res_add_fwd`` for the last conv
    of a block with its QuantAdd, ReLU and the next block's quantizers) -> ``mn_i8_unpack_codes`` at avg_pool's scale -> the model's own avg_pool and fc.  Eval only;
    owns the packed tables and one set of byte buffers per input shape.  ``layers[i]`` keeps what stage i was packed from (w, s_w, bias, s_a, s_add, s_out per output
    map, the widths, src / sc / outs buffer numbers) for the tests' judge; ``buffers[b]`` is the channel count of code map b; ``stem`` the packs behind conv1.

    A plan compiled with ``end_to_end=True`` (``ends`` is set) runs neither the model's own conv1 nor its avg_pool and fc: ``mn_i8first_fwd2`` takes the fp32 image to
    the stem's code maps, the stages run unchanged, ``mn_i8poolfc_fwd`` takes the last block's codes to the fp32 logits (``csrc/qgemm_iao8_e2e.h``): no pack, no unpack,
    no fp32 activation map.  ``ends`` = (first, last) keeps what the two tables were packed from (first: w, s_w, bias, s_a, s_out and out_bits per output map, in_bits,
    w_bits; last: w, s_w, bias, s_p, s_fc, p_bits, a_bits, w_bits) for the tests' judge.  Its ``report`` is the walk's at 32 x 32 until the plan runs, then that of
    the image size it last ran on (``iao_int8_report(model, (H, W), end_to_end=True)``: the activation bytes, and whether the pooled map fits, depend on it)."""

    who = "iao_compile_int8"

    def __init__(self, conv1, stages, avg_pool, fc, report, stem, buffers, tail, ends=None, report_of=None):
        super().__init__(conv1, stages, None, [avg_pool, fc], True, report)
        self.stem, self.buffers, self.tail_q = stem, buffers, tail          # tail: dict(buf, s, C)
        self.ends = ends                  # None, or the layer dicts (first, last) of an end_to_end plan
        self._report_of, self._reports = report_of, {}          # end_to_end: (H, W) -> the report at that image size
        self.stage_codes = []

    def _plan_buffers(self, shape, device):
        """Every code map, the geometry of every stage and the fp32 map in front of avg_pool for one conv1 output shape."""
        N, Cc, H, W = shape
        if Cc != self.stem["cout"]:
            raise _err("iao_compile_int8: conv1 produced %d channels, the first block reads %d" % (Cc, self.stem["cout"]))
        dims = {o["buf"]: (H, W) for o in self.stem["outs"]}
        geoms = []
        for L in self.layers:
            h, w = dims[L["src"]]
            geoms.append(_block_geom(L, N, h, w))
            for o in L["outs"]:
                dims[o["buf"]] = ((h - 1) // L["stride"] + 1, (w - 1) // L["stride"] + 1)
        bufs = [_code_map(N, c, dims[b][0] * dims[b][1], device) for b, c in enumerate(self.buffers)]
        ht, wt = dims[self.tail_q["buf"]]
        if self.ends:          # the logits, and the pooled map's size in place of an fp32 map
            return bufs, geoms, (torch.empty((N, self.ends[1]["cout"]), dtype=torch.float32, device=device), ht * wt)
        return bufs, geoms, torch.empty((N, self.tail_q["C"], ht, wt), dtype=torch.float32, device=device)

    def _launch(self, L, g, src, sc, outs, st):
        from micronet_amd import _lib, ops
        if L["api"] == "i8conv":
            ops._call("mn_i8conv_fwd", C.byref(g), L["a_bits"], L["w_bits"], ops._p(L["table"]), ops._p(src), ops._p(outs[0]), 0, st)
        elif L["api"] == "res_conv":
            ops._call("mn_i8res_conv_fwd", C.byref(g), L["in_bits"], L["a_bits"], L["w_bits"], ops._p(L["table"]), ops._p(src), ops._p(outs[0]), L["relu"], st)
        else:
            q = _two_outs(_lib.I8ResAdd(), L, len(L["outs"]))
            q.s_add, q.add_bits = L["s_add"], L["a_bits"]
            ops._call("mn_i8res_add_fwd", C.byref(g), L["in_bits"], L["w_bits"], ops._p(L["table"]), ops._p(src), ops._p(sc), C.byref(q), ops._p(outs[0]),
                      ops._p(outs[1]) if len(outs) == 2 else None, st)

    def run_stage(self, i, codes, N, H, W, shortcut=None):
        """Stage ``i`` alone on blocked input codes [N, ceil(cin / 16), H * W, 16] (int8, GPU; an add stage also takes the shortcut's codes [N, ceil(cout / 16), H * W, 16]):
        the list of its blocked output maps, freshly allocated and poisoned (tests)."""
        from micronet_amd import ops
        L = self.layers[i]
        Ho, Wo = (H - 1) // L["stride"] + 1, (W - 1) // L["stride"] + 1
        if (not _is_code_map(codes, N, L["cin"], H * W) or (L["api"] == "res_add") != (shortcut is not None)
                or (shortcut is not None and not _is_code_map(shortcut, N, L["cout"], Ho * Wo))):
            raise _err("iao_compile_int8: run_stage needs int8 GPU codes [N, ceil(C / 16), H * W, 16] (and the shortcut's codes for an add stage, for no other)")
        outs = [_code_map(N, L["cout"], Ho * Wo, codes.device, fill=77) for _ in L["outs"]]
        with torch.cuda.device(codes.device):
            self._launch(L, _block_geom(L, N, H, W), codes.contiguous(), shortcut.contiguous() if shortcut is not None else None, outs, ops._s())
        return outs

    def _first(self, x, outs, st):
        from micronet_amd import _lib, ops
        Lf, (N, _, H, W) = self.ends[0], x.shape
        q = _two_outs(_lib.I8FirstOuts(), Lf, len(outs))
        ops._call("mn_i8first_fwd2", C.byref(_block_geom(Lf, N, H, W)), Lf["in_bits"], Lf["w_bits"], ops._p(Lf["table"]), ops._p(x), C.byref(q), ops._p(outs[0]),
                  ops._p(outs[1]) if len(outs) == 2 else None, st)

    def _last(self, codes, N, HW, y, st):
        from micronet_amd import ops
        Ll = self.ends[1]
        ops._call("mn_i8poolfc_fwd", N, Ll["cin"], HW, Ll["cout"], Ll["p_bits"], Ll["a_bits"], Ll["w_bits"], ops._p(Ll["table"]), ops._p(codes), ops._p(y), st)

    def run_first(self, x):
        """conv1 alone on the fp32 image (end_to_end): the list of the blocked code maps [N, ceil(cout / 16), H * W, 16] the first block reads, one per consumer
        quantizer, freshly allocated and poisoned (tests)."""
        from micronet_amd import ops
        x = _iao8_ends_image(self.ends, x, "end_to_end")
        Lf, (N, _, H, W) = self.ends[0], x.shape
        outs = [_code_map(N, Lf["cout"], H * W, x.device, fill=77) for _ in Lf["outs"]]
        with torch.cuda.device(x.device):
            self._first(x, outs, ops._s())
        return outs

    def run_last(self, codes, N, H, W):
        """avg_pool and fc alone on the last block's blocked codes [N, ceil(cin / 16), H * W, 16] (end_to_end): the fp32 logits [N, cout], freshly allocated and
        poisoned (tests)."""
        from micronet_amd import ops
        Ll, codes = _iao8_ends_codes(self.ends, codes, N, H, W, "end_to_end")
        y = torch.full((N, Ll["cout"]), float("nan"), dtype=torch.float32, device=codes.device)
        with torch.cuda.device(codes.device):
            self._last(codes, N, H * W, y, ops._s())
        return y

    def _forward_ends(self, x):
        from micronet_amd import ops
        x = _iao8_ends_image(self.ends, x, "end_to_end")
        N, _, H, W = x.shape
        if (H, W) not in self._reports:
            self._reports[(H, W)] = self._report_of((H, W))          # (raises where the pooled map of this image size is not covered)
        self.report = self._reports[(H, W)]
        with torch.cuda.device(x.device):
            bufs, geoms, (y, hw) = self._shape_buffers((N, self.stem["cout"], H, W), x.device)          # (stride 1, padding (k - 1) / 2: conv1 keeps H x W)
            st = ops._s()
            self._first(x, [bufs[o["buf"]] for o in self.stem["outs"]], st)
            for L, g in zip(self.layers, geoms):
                self._launch(L, g, bufs[L["src"]], bufs[L["sc"]] if L["sc"] is not None else None, [bufs[o["buf"]] for o in L["outs"]], st)
            if self.keep_stages:
                self.stage_codes = [b.clone() for b in bufs]
            self._last(bufs[self.tail_q["buf"]], N, hw, y, st)
        return y.clone()          # (the buffer belongs to the plan: never handed out)

    @torch.no_grad()
    def forward(self, x):
        from micronet_amd import ops
        if self.ends:
            return self._forward_ends(x)
        a = self.first(x)
        if not (type(a) is torch.Tensor and a.is_cuda and a.dtype == torch.float32 and a.dim() == 4):
            raise _err("iao_compile_int8: conv1 did not produce a float32 GPU map (the input must be a float32 GPU tensor; no CPU fallback)")
        a = a.contiguous()
        N, Cc, H, W = a.shape
        with torch.cuda.device(a.device):
            bufs, geoms, y = self._shape_buffers(a.shape, a.device)
            st = ops._s()
            for o in self.stem["outs"]:
                ops._call("mn_i8_pack_codes", ops._p(a), N, Cc, H * W, o["s"], o["bits"], None, ops._p(bufs[o["buf"]]), st)
            for L, g in zip(self.layers, geoms):
                self._launch(L, g, bufs[L["src"]], bufs[L["sc"]] if L["sc"] is not None else None, [bufs[o["buf"]] for o in L["outs"]], st)
            if self.keep_stages:
                self.stage_codes = [b.clone() for b in bufs]
            n_, c_, h_, w_ = y.shape
            ops._call("mn_i8_unpack_codes", ops._p(bufs[self.tail_q["buf"]]), n_, c_, h_ * w_, self.tail_q["s"], ops._p(y), st)
        y = self.tail[0](y)
        return self.tail[1](y.view(y.size(0), -1))


@torch.no_grad()
def _compile_iao8_res(model, byte_ends=False, end_to_end=False):
    import math
    from micronet_amd import ops
    who = "iao_compile_int8(end_to_end=True)" if end_to_end else "iao_compile_int8"
    stem, stages, buffers, tail_q, report = _walk_iao8_res(model, byte_ends=byte_ends, end_to_end=end_to_end)
    ends = stem.pop("ends", None)
    _require_gpu(model, who)
    dev = stages[0]["conv"].weight.device
    # every scale the plan needs, in ONE host read
    qs = [o["q"] for o in stem["outs"]]
    for L in stages:
        qs += [L["conv"].activation_quantizer] + [o["q"] for o in L["outs"]] + ([L["add"]] if "add" in L else [])
    if ends:
        qs += [ends[0]["conv"].activation_quantizer, ends[1]["fc"].activation_quantizer]
    scale = {i: s for i, (s, _) in _iao8_constants(qs).items()}
    for o in stem["outs"]:
        q = o.pop("q")
        o["s"], o["bits"] = scale[id(q)], q.bits
    with torch.cuda.device(dev):
        for L in stages:
            conv = L.pop("conv")
            _iao8_packed_from(L, conv, dev)
            L["s_a"] = scale[id(conv.activation_quantizer)]
            L["s_out"] = [scale[id(o.pop("q"))] for o in L["outs"]]
            L["s_add"] = scale[id(L.pop("add"))] if "add" in L else None
            s_tab = L["s_add"] if L["api"] == "res_add" else L["s_out"][0]          # the scale of the codes the conv's epilogue forms
            if L["api"] == "i8conv":
                ops._call("mn_i8conv_pack", C.byref(_block_geom(L)), ops._p(L["w"]), ops._p(L["s_w"]), 1 if L["per_channel"] else 0, ops._p(L["bias"]), L["s_a"], s_tab, s_tab,
                          L["a_bits"], L["w_bits"], None, ops._p(L["table"]), ops._s())
            else:
                ops._call("mn_i8res_pack", C.byref(_block_geom(L)), ops._p(L["w"]), ops._p(L["s_w"]), 1 if L["per_channel"] else 0, ops._p(L["bias"]), L["s_a"], s_tab,
                          L["in_bits"], L["a_bits"], L["w_bits"], ops._p(L["table"]), ops._s())
        if ends:
            Lf, Ll = ends
            conv, fc = Lf.pop("conv"), Ll.pop("fc")
            _iao8_packed_from(Lf, conv, dev)
            _iao8_packed_from(Ll, fc, dev)
            Lf["s_a"], Lf["s_out"] = scale[id(conv.activation_quantizer)], [o["s"] for o in stem["outs"]]
            ops._call("mn_i8first_pack", C.byref(_block_geom(Lf)), ops._p(Lf["w"]), ops._p(Lf["s_w"]), 1 if Lf["per_channel"] else 0, ops._p(Lf["bias"]), Lf["s_a"],
                      Lf["s_out"][0], Lf["in_bits"], Lf["out_bits"][0], Lf["w_bits"], None, ops._p(Lf["table"]), ops._s())
            Ll["s_p"], Ll["s_fc"] = stages[-1]["s_out"][0], scale[id(fc.activation_quantizer)]
            ops._call("mn_i8poolfc_pack", Ll["cin"], Ll["cout"], ops._p(Ll["w"]), ops._p(Ll["s_w"]), 1 if Ll["per_channel"] else 0, ops._p(Ll["bias"]), Ll["s_p"], Ll["s_fc"],
                      Ll["p_bits"], Ll["a_bits"], Ll["w_bits"], ops._p(Ll["table"]), ops._s())
        packed = stages + (list(ends) if ends else [])
        counters = _iao8_counters(packed)          # ... and every table's counters in one more
    for L, row in zip(packed, counters):
        _iao8_check_counters(who, L["name"], L, row, "s_a, s_out")
        for s in L.get("s_out", []) + ([L["s_add"]] if L.get("s_add") is not None else []):
            if not (math.isfinite(s) and s > 0):
                raise _err("%s: %s: a consumer's scale %r is not finite and positive" % (who, L["name"], s))
    last = stages[-1]
    tail = dict(buf=last["outs"][0]["buf"], s=last["s_out"][0], C=last["cout"])
    report_of = (lambda hw: _walk_iao8_res(model, hw, end_to_end=True)[4]) if ends else None
    return Int8ResPlan(model.conv1, stages, model.avg_pool, model.fc, report, stem, buffers, tail, ends, report_of)
