"""Reference and rounding model of one whole pass of the convolutional image towers — cnx_forward (csrc/convnext.hip) and rn_forward (csrc/resnet.hip) —
for tests/test_convtower_ref_host.py and tests/test_convtower_forms_gpu.py.  A plain helper module in the style of tests/encoder_ref.py: nothing here
calls the library, and everything runs on the device of its input.

Every kernel those walks launch has its own budgeted float64 parity test (tests/test_conv_kernels_gpu.py, tests/test_gemm_parity_gpu.py,
tests/test_rowops_gpu.py).  What is held to account HERE is the host-side glue between them: the LayerNorm, layer-scale and BatchNorm folds, the stride
and downsample ordering, the 2x2 average pool of both branches, the channel padding to multiples of 64, the X / D buffer swap and the in-place residual
GEMMs, the workspace plan and the attention-pool wiring.

    convnext_operands(arch, sd) / resnet_operands(arch, sd)    the operands as engine/towers.py (ConvNextTower, ResNetTower) hands them to the library, built
                                                               with the load-time folds of engine/tower_weights.py: bf16-rounded matrices, fp32 vectors — in
                                                               float64.  round_matrices=False leaves the matrices un-rounded (the pin to the fp32 restatements)
    convnext_exact / resnet_exact (arch, ops, pixels)          rounds nothing
    convnext_model / resnet_model (arch, ops, pixels, mut)     the same code, rounding to bf16 / fp32 exactly where the walk stores bf16 / fp32; `mut`: ONE
                                                               deliberate defect (CNX_MUTATIONS, RN_MUTATIONS)
both return (the un-normalised output [n, E], the last stage's per-pixel stream [n H3 H3, C3]).  `pixels`: the NORMALISED fp32 pixels [n, 3, S, S] (what
the f32 entry points take; for the u8 entry points normalise(u8) evaluates the kernels' fp32 expression (b / 255 - mean) / std).  The judge is
encoder_ref.row_ratio: per row, the larger of |got - exact| / |model - exact| in the 2-norm and in the max-norm, against the project's MARGIN.

Where cnx_forward stores (x: the stream, y: the second stream-sized buffer, h: the hidden buffer):
    h = bf16(patch matrix)   y = bf16(h stem_w^T + b)   x = bf16(LN y)                                            (the stem; LN statistics of the bf16 rows)
    y = bf16(dwconv7(x) + b)   h = bf16(GELU(rstd (y wf^T - mean colsum) + bf))   x = bf16(x + h w2^T + b2)       (a block: LN folded into fc1, gamma into fc2;
                                                                                                                  the statistics are those of the bf16 rows y)
    y = bf16(LN x) gathered 2x2 in (ky, kx, c) order   x = bf16(y ds_w^T + b)                                     (a downsample)
    pooled = bf16(LN(mean over the pixels of x))   [hid = bf16(GELU(pooled p1^T + b1))]   out = fp32(...)         (the head)
Where rn_forward stores (every activation is a bf16 [pixels, channels] buffer):
    A = bf16(27 stem taps)   B = bf16(relu(A w^T + b))   A = bf16(relu(conv3x3 B))   B = bf16(relu(conv3x3 A))   X = bf16(avgpool2 B)
    A = bf16(relu(X c1^T + b))   B = bf16(relu(conv3x3 A))   [A = bf16(avgpool2 B), Cb = bf16(avgpool2 X)]
    [D = bf16(xin ds^T + b)]   X = bf16(relu(main c3^T + b + identity))                                           (ReLU after the residual add)
    tokens = bf16(mean + pos[0]), bf16(x + pos[1 + p])   kv = bf16(tokens kv_w^T + b)   q = bf16(token 0 q_w^T + b)   (q_w carries 64^-0.5)
    attention: fp32 scores, fp32 probabilities, the quotient stored as bf16 (tests/conv_ref.py: reference_attend / model_attend, reused here)
    out = fp32(a c_w^T + c_b)
Channels padded to a multiple of 64 (the stem's output and the blocks' inner width) are carried explicitly, with the zero weight rows / columns and zero
biases the loader writes, so that the reference walks the same widths as the library.
"""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from marqo_amd.engine import tower_weights as TW
from marqo_amd.engine.archs import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD
from tests import conv_ref
from tests.encoder_ref import ZeroYardstick, row_ratio      # noqa: F401  (re-exported: the judge of both test files)
from tests.test_patch_attn_gpu import MARGIN                # noqa: F401  (the project's factor between two rounding histories)

Tensor = torch.Tensor
F64 = torch.float64

CNX_MUTATIONS = ("gamma_dropped", "eps_swapped", "dw_border_replicated", "ds_taps_xy", "pool_divisor", "pool_positions", "quick_gelu")
RN_MUTATIONS = ("relu_before_add", "identity_not_pooled", "avgpool_divisor", "pad_not_zero", "pad_nan", "no_positions", "q_unscaled", "images_swapped",
                "ds_by_padded_width")


# ---- the fp32 restatements the full-size GPU tests compare with (tests/test_convnext_gpu.py, tests/test_resnet_gpu.py); they run on the device of `x` ----
def _torch_trunk(sd, arch, x):
    """the timm trunk restated in torch fp32 (NCHW), any LayerNorm eps -> the pooled, normed [n, C3] row"""
    t, eps = "visual.trunk.", arch.ln_eps
    p = lambda k: sd[t + k].to(x.device)

    def ln_cf(x, name):
        return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), p(name + ".weight"), p(name + ".bias"), eps).permute(0, 3, 1, 2)

    x = ln_cf(F.conv2d(x, p("stem.0.weight"), p("stem.0.bias"), stride=4), "stem.1")
    for i, depth in enumerate(arch.depths):
        s = f"stages.{i}."
        if i > 0:
            x = F.conv2d(ln_cf(x, s + "downsample.0"), p(s + "downsample.1.weight"), p(s + "downsample.1.bias"), stride=2)
        for j in range(depth):
            b = f"{s}blocks.{j}."
            C = x.shape[1]
            y = F.conv2d(x, p(b + "conv_dw.weight"), p(b + "conv_dw.bias"), padding=3, groups=C).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (C,), p(b + "norm.weight"), p(b + "norm.bias"), eps)
            y = F.linear(F.gelu(F.linear(y, p(b + "mlp.fc1.weight"), p(b + "mlp.fc1.bias"))), p(b + "mlp.fc2.weight"), p(b + "mlp.fc2.bias"))
            x = x + (y * p(b + "gamma")).permute(0, 3, 1, 2)
    return F.layer_norm(x.mean((2, 3)), (x.shape[1],), p("head.norm.weight"), p("head.norm.bias"), eps)


def _head(sd, arch, pooled):
    dev = pooled.device
    if arch.head == "linear":
        return F.linear(pooled, sd["visual.head.proj.weight"].to(dev))
    h = F.gelu(F.linear(pooled, sd["visual.head.mlp.fc1.weight"].to(dev), sd["visual.head.mlp.fc1.bias"].to(dev)))
    b2 = sd.get("visual.head.mlp.fc2.bias")
    return F.linear(h, sd["visual.head.mlp.fc2.weight"].to(dev), None if b2 is None else b2.to(dev))


def _torch_resnet(sd, arch, x):
    """OpenAI CLIP's ModifiedResNet (= open_clip's) in fp32, NCHW, eval mode -> attnpool output [n, E]"""
    p = lambda k: sd[k].to(x.device).float()
    v = "visual."

    def bn(t, name):
        return F.batch_norm(t, p(name + ".running_mean"), p(name + ".running_var"), p(name + ".weight"), p(name + ".bias"), False, 0.0, 1e-5)

    x = F.relu(bn(F.conv2d(x, p(v + "conv1.weight"), stride=2, padding=1), v + "bn1"))
    x = F.relu(bn(F.conv2d(x, p(v + "conv2.weight"), padding=1), v + "bn2"))
    x = F.relu(bn(F.conv2d(x, p(v + "conv3.weight"), padding=1), v + "bn3"))
    x = F.avg_pool2d(x, 2)
    for i, depth in enumerate(arch.layers):
        for j in range(depth):
            b = f"{v}layer{i + 1}.{j}."
            stride = 2 if (i > 0 and j == 0) else 1
            out = F.relu(bn(F.conv2d(x, p(b + "conv1.weight")), b + "bn1"))
            out = F.relu(bn(F.conv2d(out, p(b + "conv2.weight"), padding=1), b + "bn2"))
            if stride > 1:
                out = F.avg_pool2d(out, stride)
            out = bn(F.conv2d(out, p(b + "conv3.weight")), b + "bn3")
            idn = x
            if b + "downsample.0.weight" in sd:
                idn = bn(F.conv2d(F.avg_pool2d(x, stride) if stride > 1 else x, p(b + "downsample.0.weight")), b + "downsample.1")
            x = F.relu(out + idn)
    n, C = x.shape[:2]
    t = x.flatten(2).permute(2, 0, 1)
    t = torch.cat([t.mean(0, keepdim=True), t]) + p(v + "attnpool.positional_embedding")[:, None, :]
    a = v + "attnpool."
    out, _ = F.multi_head_attention_forward(
        query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=C // 64, q_proj_weight=p(a + "q_proj.weight"),
        k_proj_weight=p(a + "k_proj.weight"), v_proj_weight=p(a + "v_proj.weight"), in_proj_weight=None,
        in_proj_bias=torch.cat([p(a + "q_proj.bias"), p(a + "k_proj.bias"), p(a + "v_proj.bias")]), bias_k=None, bias_v=None,
        add_zero_attn=False, dropout_p=0.0, out_proj_weight=p(a + "c_proj.weight"), out_proj_bias=p(a + "c_proj.bias"),
        use_separate_proj_weight=True, training=False, need_weights=False)
    return out[0]


# ---- inputs and stores -----------------------------------------------------------------------------------------------------------------------
def normalise(u8: Tensor, mean=OPENAI_DATASET_MEAN, std=OPENAI_DATASET_STD) -> Tensor:
    """uint8 [n, S, S, 3] -> fp32 [n, 3, S, S]: (b / 255 - mean) / std in fp32, the expression of mq_patchify and mq_resnet_stem_gather"""
    m = torch.tensor(mean, dtype=torch.float32, device=u8.device).view(1, 1, 1, 3)
    s = torch.tensor(std, dtype=torch.float32, device=u8.device).view(1, 1, 1, 3)
    return ((u8.float() / 255.0 - m) / s).permute(0, 3, 1, 2).contiguous()


class _Round:
    """the two stores of a walk; the exact reference stores nothing"""

    def __init__(self, on: bool):
        self.on = on

    def b(self, t: Tensor) -> Tensor:
        return t.float().to(torch.bfloat16).to(F64) if self.on else t

    def f(self, t: Tensor) -> Tensor:
        return t.float().to(F64) if self.on else t


def _w(t: Tensor, rounded: bool) -> Tensor:
    t = t.detach().float()
    return (t.to(torch.bfloat16) if rounded else t).to(F64)


def _v(t: Tensor) -> Tensor:
    return t.detach().float().to(F64)


def ops_to(ops, device):
    if isinstance(ops, Tensor):
        return ops.to(device)
    if isinstance(ops, dict):
        return {k: ops_to(v, device) for k, v in ops.items()}
    if isinstance(ops, (list, tuple)):
        return type(ops)(ops_to(v, device) for v in ops)
    return ops


def _stats(x: Tensor, eps: float):
    mean = x.mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)


def _ln(x: Tensor, g: Tensor, b: Tensor, eps: float) -> Tensor:
    mean, rstd = _stats(x, eps)
    return (x - mean) * rstd * g + b


def _gelu(x: Tensor) -> Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _quick_gelu(x: Tensor) -> Tensor:
    return x * torch.sigmoid(1.702 * x)


# ---- ConvNeXt ---------------------------------------------------------------------------------------------------------------------------------
def convnext_operands(arch, sd: Dict[str, Tensor], round_matrices: bool = True) -> dict:
    """what ConvNextTower hands to mq_encode_convnext_*, in float64 on the CPU.  Per block also `fc2_w_plain` / `fc2_b_plain`: fc2 WITHOUT the layer scale
    (the gamma_dropped mutation)"""
    t, dims, r = "visual.trunk.", arch.dims, round_matrices
    f32 = lambda k: sd[k].detach().float()
    C0 = dims[0]
    ops = dict(stem_w=_w(f32(t + "stem.0.weight").reshape(C0, 48), r), stem_b=_v(f32(t + "stem.0.bias")), stem_ln_g=_v(f32(t + "stem.1.weight")),
               stem_ln_b=_v(f32(t + "stem.1.bias")), ds=[None] * 4, blocks=[])
    for i, (depth, Ch) in enumerate(zip(arch.depths, dims)):
        p = f"{t}stages.{i}."
        if i > 0:
            ops["ds"][i] = dict(ln_g=_v(f32(p + "downsample.0.weight")), ln_b=_v(f32(p + "downsample.0.bias")),
                                w=_w(TW.convnext_downsample_weight(f32(p + "downsample.1.weight")), r), b=_v(f32(p + "downsample.1.bias")))
        for j in range(depth):
            b = f"{p}blocks.{j}."
            w1, b1, g1, be1 = f32(b + "mlp.fc1.weight"), f32(b + "mlp.fc1.bias"), f32(b + "norm.weight"), f32(b + "norm.bias")
            wf, bf, sf = TW.convnext_fold_ln_fc1(w1, b1, g1, be1)
            if r:
                fc1_w, fc1_s = wf.to(F64), _v(sf)
            else:
                fc1_w = w1.to(F64) * g1.to(F64)[None, :]
                fc1_s = fc1_w.sum(1)
            w2, b2 = TW.convnext_fold_gamma_fc2(f32(b + "mlp.fc2.weight"), f32(b + "mlp.fc2.bias"), f32(b + "gamma"))
            ops["blocks"].append(dict(stage=i, dw_w=_v(TW.convnext_dw_taps(f32(b + "conv_dw.weight"))), dw_b=_v(f32(b + "conv_dw.bias")), fc1_w=fc1_w,
                                      fc1_b=_v(bf), fc1_s=fc1_s, fc2_w=_w(w2, r), fc2_b=_v(b2), fc2_w_plain=_w(f32(b + "mlp.fc2.weight"), r),
                                      fc2_b_plain=_v(f32(b + "mlp.fc2.bias"))))
    ops["head_ln_g"], ops["head_ln_b"] = _v(f32(t + "head.norm.weight")), _v(f32(t + "head.norm.bias"))
    if arch.head == "linear":
        ops["proj_w"] = _w(f32("visual.head.proj.weight"), r)
    else:
        ops["proj_w"], ops["proj_b"] = _w(f32("visual.head.mlp.fc1.weight"), r), _v(f32("visual.head.mlp.fc1.bias"))
        ops["proj2_w"] = _w(f32("visual.head.mlp.fc2.weight"), r)
        ops["proj2_b"] = _v(f32("visual.head.mlp.fc2.bias")) if "visual.head.mlp.fc2.bias" in sd else None
    return ops


def _dwconv7(x: Tensor, taps: Tensor, bias: Tensor, replicate: bool) -> Tensor:
    """x [n, H, W, C], taps [49, C] (tap ky * 7 + kx) -> [n, H, W, C]; outside the image: zeros, or (replicate) the nearest border pixel"""
    n, H, W, C = x.shape
    out = bias.expand(n, H, W, C).clone()
    ys, xs = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
    for ky in range(7):
        iy = ys + ky - 3
        oky = (iy >= 0) & (iy < H)
        rows = x[:, iy.clamp(0, H - 1)]
        for kx in range(7):
            ix = xs + kx - 3
            okx = (ix >= 0) & (ix < W)
            term = rows[:, :, ix.clamp(0, W - 1)] * taps[ky * 7 + kx]
            if not replicate:
                term = term * (oky[:, None] & okx[None, :])[None, :, :, None]
            out = out + term
    return out


def _cnx_run(arch, ops: dict, pixels: Tensor, R: _Round, mut: Optional[str] = None):
    assert mut is None or mut in CNX_MUTATIONS, mut
    assert pixels.dtype == torch.float32 and pixels.dim() == 4 and pixels.shape[1] == 3
    n, S = pixels.shape[0], arch.image_size
    H = S // 4
    eps = arch.ln_eps
    if mut == "eps_swapped":
        eps = 1e-5 if eps == 1e-6 else 1e-6
    act = _quick_gelu if mut == "quick_gelu" else _gelu
    px = pixels.to(F64)
    # stem: the 4x4 patches as rows of (c, ky, kx) columns -> GEMM + bias -> LayerNorm
    h = R.b(px.reshape(n, 3, H, 4, H, 4).permute(0, 2, 4, 1, 3, 5).reshape(n * H * H, 48))
    y = R.b(h @ ops["stem_w"].T + ops["stem_b"])
    x = R.b(_ln(y, ops["stem_ln_g"], ops["stem_ln_b"], eps))
    C = arch.dims[0]
    blocks = ops["blocks"]
    dropped = len(blocks) // 2      # gamma_dropped: the block in the middle of the walk
    k = 0
    for st in range(4):
        if st > 0:
            d = ops["ds"][st]
            t = R.b(_ln(x, d["ln_g"], d["ln_b"], eps)).reshape(n, H // 2, 2, H // 2, 2, C)
            t = t.permute(0, 1, 3, 4, 2, 5) if mut == "ds_taps_xy" else t.permute(0, 1, 3, 2, 4, 5)       # (ky, kx, c) columns
            H //= 2
            x = R.b(t.reshape(n * H * H, 4 * C) @ d["w"].T + d["b"])
            C = arch.dims[st]
        for _ in range(arch.depths[st]):
            b = blocks[k]
            y = R.b(_dwconv7(x.reshape(n, H, H, C), b["dw_w"], b["dw_b"], replicate=(mut == "dw_border_replicated" and st == 0))).reshape(n * H * H, C)
            mean, rstd = _stats(y, eps)
            hid = R.b(act(rstd * (y @ b["fc1_w"].T - mean * b["fc1_s"][None, :]) + b["fc1_b"]))
            w2, b2 = (b["fc2_w_plain"], b["fc2_b_plain"]) if (mut == "gamma_dropped" and k == dropped) else (b["fc2_w"], b["fc2_b"])
            x = R.b(x + hid @ w2.T + b2)
            k += 1
    HW = H * H
    xs = x.reshape(n, HW, C)
    if mut == "pool_positions":     # the pool leaves the last position out
        xs = xs[:, :HW - 1]
    m = xs.sum(1) / (HW + 1 if mut == "pool_divisor" else HW)
    pooled = R.b(_ln(m, ops["head_ln_g"], ops["head_ln_b"], eps))
    if arch.head == "linear":
        out = R.f(pooled @ ops["proj_w"].T)
    else:
        hid = R.b(act(pooled @ ops["proj_w"].T + ops["proj_b"]))
        out = hid @ ops["proj2_w"].T
        out = R.f(out + ops["proj2_b"] if ops["proj2_b"] is not None else out)
    return out, x


def convnext_exact(arch, ops: dict, pixels: Tensor):
    return _cnx_run(arch, ops, pixels, _Round(False))


def convnext_model(arch, ops: dict, pixels: Tensor, mut: Optional[str] = None):
    return _cnx_run(arch, ops, pixels, _Round(True), mut)


# ---- ResNet -------------------------------------------------------------------------------------------------------------------------------------
def resnet_operands(arch, sd: Dict[str, Tensor], round_matrices: bool = True) -> dict:
    """what ResNetTower hands to mq_encode_resnet_*, in float64 on the CPU: every BatchNorm folded, every width padded as the loader pads it.  `q_w_plain` /
    `q_b_plain`: q_proj WITHOUT the 64^-0.5 softmax scale (the q_unscaled mutation)"""
    v, w0, r = "visual.", arch.width, round_matrices
    f32 = lambda k: sd[k].detach().float()

    def conv_bn(conv, bn):
        return TW.resnet_fold_bn(f32(conv + ".weight"), f32(bn + ".weight"), f32(bn + ".bias"), f32(bn + ".running_mean"), f32(bn + ".running_var"))

    c1, wp = w0 // 2, TW.resnet_pad64(w0)
    ops: dict = dict(stem=[], blocks=[])
    a, b = conv_bn(v + "conv1", v + "bn1")
    ops["stem"].append((_w(TW.resnet_stem_weight(a), r), _v(b)))
    a, b = conv_bn(v + "conv2", v + "bn2")
    ops["stem"].append((_w(TW.resnet_conv3x3_weight(a, c1, c1), r), _v(b)))
    a, b = conv_bn(v + "conv3", v + "bn3")
    ops["stem"].append((_w(TW.resnet_conv3x3_weight(a, c1, wp), r), _v(TW.resnet_pad_vec(b, wp))))
    inp = w0
    for i, depth in enumerate(arch.layers):
        P = w0 << i
        Pp, O = TW.resnet_pad64(P), 4 * P
        for j in range(depth):
            p = f"{v}layer{i + 1}.{j}."
            ip = TW.resnet_pad64(inp)
            blk = dict(stage=i, down=(i > 0 and j == 0), inp=ip, P=Pp, out=O, real_P=P, real_inp=inp)
            a, b = conv_bn(p + "conv1", p + "bn1")
            blk["conv1_w"], blk["conv1_b"] = _w(TW.resnet_conv1x1_weight(a, ip, Pp), r), _v(TW.resnet_pad_vec(b, Pp))
            a, b = conv_bn(p + "conv2", p + "bn2")
            blk["conv2_w"], blk["conv2_b"] = _w(TW.resnet_conv3x3_weight(a, Pp, Pp), r), _v(TW.resnet_pad_vec(b, Pp))
            a, b = conv_bn(p + "conv3", p + "bn3")
            blk["conv3_w"], blk["conv3_b"] = _w(TW.resnet_conv1x1_weight(a, Pp, O), r), _v(b)
            blk["ds_w"] = None
            if p + "downsample.0.weight" in sd:       # (the checkpoint decides, as in the module: the first block of every stage)
                a, b = conv_bn(p + "downsample.0", p + "downsample.1")
                blk["ds_w"], blk["ds_b"] = _w(TW.resnet_conv1x1_weight(a, ip, O), r), _v(b)
            ops["blocks"].append(blk)
            inp = O
    apw = TW.resnet_attnpool_weights(sd, arch)
    ap = v + "attnpool."
    ops.update(pos=_v(apw["pos"]), q_w=_w(apw["q_w"], r), q_b=_v(apw["q_b"]), kv_w=_w(apw["kv_w"], r), kv_b=_v(apw["kv_b"]), c_w=_w(apw["c_w"], r),
               c_b=_v(apw["c_b"]), q_w_plain=_w(f32(ap + "q_proj.weight"), r), q_b_plain=_v(f32(ap + "q_proj.bias")), c1=c1, wp=wp, real_w=w0)
    return ops


def _conv3x3(x: Tensor, wk: Tensor, bias: Tensor) -> Tensor:
    """x [n, H, W, Cin], wk [Cout, Kp] with column (ky * 3 + kx) * Cin + c (the K padding is not read) -> [n, H, W, Cout], zero padding"""
    n, H, W, Cin = x.shape
    xp = torch.zeros(n, H + 2, W + 2, Cin, dtype=x.dtype, device=x.device)
    xp[:, 1:-1, 1:-1] = x
    out = bias.expand(n * H * W, wk.shape[0]).clone()
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            out = out + xp[:, ky:ky + H, kx:kx + W].reshape(n * H * W, Cin) @ wk[:, t * Cin:(t + 1) * Cin].T
    return out.reshape(n, H, W, -1)


def _avgpool2(x: Tensor, divisor: float = 4.0) -> Tensor:
    return (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) / divisor


def _attend(q: Tensor, kv: Tensor, R: _Round) -> Tensor:
    """q [n, C], kv [n, T, 2 C] (values the kernel reads as bf16) -> [n, C].  tests/conv_ref.py: the float64 reference, and — where the walk rounds — the
    fp32 model of ap_attend_kernel (fp32 scores and probabilities, the quotient stored as bf16), which runs on the CPU"""
    if not R.on:
        n, T, C2 = kv.shape
        C, Hh = C2 // 2, C2 // 128
        qd = q.reshape(n, Hh, 1, 64)
        k = kv[..., :C].reshape(n, T, Hh, 64).transpose(1, 2)
        v = kv[..., C:].reshape(n, T, Hh, 64).transpose(1, 2)
        return (torch.softmax((qd * k).sum(-1), -1)[..., None] * v).sum(2).reshape(n, C)
    out = conv_ref.model_attend(q.float().cpu(), kv.float().cpu())
    return torch.from_numpy(out).to(q.device).to(F64)


def _rn_run(arch, ops: dict, pixels: Tensor, R: _Round, mut: Optional[str] = None):
    assert mut is None or mut in RN_MUTATIONS, mut
    assert pixels.dtype == torch.float32 and pixels.dim() == 4 and pixels.shape[1] == 3
    n, S = pixels.shape[0], arch.image_size
    dev = pixels.device
    c1, wp, w0 = ops["c1"], ops["wp"], ops["real_w"]
    div = 3.0 if mut == "avgpool_divisor" else 4.0
    garbage = {"pad_not_zero": 1.0, "pad_nan": float("nan")}.get(mut)

    def soil(t: Tensor, real: int) -> Tensor:       # the padded channels of a buffer hold what the walk did not write
        if garbage is not None and t.shape[-1] > real:
            t = t.clone()
            t[..., real:] = garbage
        return t

    # stem: the 27 taps of the stride-2 3x3 convolution (zero outside the image, columns 27 .. 63 zero) -> GEMM, two 3x3 convolutions, the 2x2 average
    H = S // 2
    pp = torch.zeros(n, S + 2, S + 2, 3, dtype=F64, device=dev)
    pp[:, 1:-1, 1:-1] = pixels.to(F64).permute(0, 2, 3, 1)
    A = torch.zeros(n, H, H, 64, dtype=F64, device=dev)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            A[..., 3 * t:3 * t + 3] = pp[:, ky:ky + S:2, kx:kx + S:2]
    A = R.b(A)
    (w_a, b_a), (w_b, b_b), (w_c, b_c) = ops["stem"]
    B = R.b(torch.relu(A.reshape(-1, 64) @ w_a.T + b_a)).reshape(n, H, H, c1)
    A = R.b(torch.relu(_conv3x3(B, w_b, b_b)))
    B = soil(R.b(torch.relu(_conv3x3(A, w_c, b_c))), w0)
    X = R.b(_avgpool2(B, div))
    H //= 2
    for blk in ops["blocks"]:
        inp, P, out = blk["inp"], blk["P"], blk["out"]
        assert X.shape == (n, H, H, inp)
        A = soil(R.b(torch.relu(X.reshape(-1, inp) @ blk["conv1_w"].T + blk["conv1_b"])).reshape(n, H, H, P), blk["real_P"])
        main = soil(R.b(torch.relu(_conv3x3(A, blk["conv2_w"], blk["conv2_b"]))), blk["real_P"])
        xin = X
        if blk["down"]:
            main = R.b(_avgpool2(main, div))
            xin = X[:, 0::2, 0::2] if mut == "identity_not_pooled" else R.b(_avgpool2(X, div))
            H //= 2
        has_ds = blk["ds_w"] is not None
        if mut == "ds_by_padded_width":     # the walk as it was: the downsample branch decided by comparing the PADDED input width with the output width
            has_ds = blk["down"] or inp != out
        if has_ds:
            idn = R.b(xin.reshape(-1, inp) @ blk["ds_w"].T + blk["ds_b"])
        else:
            assert inp == out and not blk["down"]
            idn = xin.reshape(-1, out)
        branch = main.reshape(-1, P) @ blk["conv3_w"].T + blk["conv3_b"]
        X = R.b(torch.relu(branch) + idn if mut == "relu_before_add" else torch.relu(branch + idn)).reshape(n, H, H, out)
    C, HW = 32 * w0, H * H
    assert X.shape[-1] == C
    stream = X.reshape(n * HW, C)
    xs = X.reshape(n, HW, C)
    pos = torch.zeros_like(ops["pos"]) if mut == "no_positions" else ops["pos"]
    tok = R.b(torch.cat([xs.mean(1, keepdim=True), xs], 1) + pos)
    kv = R.b(tok @ ops["kv_w"].T + ops["kv_b"])
    q_w, q_b = (ops["q_w_plain"], ops["q_b_plain"]) if mut == "q_unscaled" else (ops["q_w"], ops["q_b"])
    q = R.b(tok[:, 0] @ q_w.T + q_b)
    a = _attend(q, kv, R)
    outp = R.f(a @ ops["c_w"].T + ops["c_b"])
    if mut == "images_swapped" and n > 1:
        outp = outp.clone()
        outp[[0, 1]] = outp[[1, 0]]
    return outp, stream


def resnet_exact(arch, ops: dict, pixels: Tensor):
    return _rn_run(arch, ops, pixels, _Round(False))


def resnet_model(arch, ops: dict, pixels: Tensor, mut: Optional[str] = None):
    return _rn_run(arch, ops, pixels, _Round(True), mut)


# ---- the configurations both test files run ---------------------------------------------------------------------------------------------------------
# The smallest at which the glue can still go wrong.  ConvNeXt: S = 32 gives maps of 8 / 4 / 2 / 1 pixels a side (every pixel lies within the 7x7 halo of
# the border), S = 64 gives 16 / 8 / 4 / 2 (border and interior); depths with a stage of two blocks early and late; both heads, the mlp head with and
# without its second bias; both LayerNorm eps of the served checkpoints.  ResNet: S = 64 is the smallest image the library takes (T = 5 tokens), S = 96
# gives T = 10 and odd 3-pixel maps; width 16: every stage padded or at the pad boundary; 64: nothing padded; 80: RN50x4's pad64(80) = 128;
# (2, 1, 2, 1) has an identity block without a downsample branch and a non-first block in a strided stage.
CNX_DIMS, CNX_E = (64, 128, 256, 512), 128
RN_E = 128
# rows up to which mq_gemm_bf16 takes the skinny kernels: one row group up to `small_m` (80), row groups up to `small_m_grouped` (320): tests/test_small_m_gpu.py
SKINNY_ROWS, GROUPED_ROWS = 80, 320
# ConvNeXt, S = 32: the last stage has n rows and so has the head — n = 321 is the first batch whose stage-3 and head GEMMs leave the skinny family.
# ResNet, S = 64: the last stage has 4 n rows, the k | v projection 5 n — n = 81 is the first batch whose stage-4 downsample GEMM (324 rows) and k | v
# GEMM (405) leave it; q and c_proj (81 rows) go from one row group to two.  (The ReLU GEMMs and the 3x3 convolutions have no skinny form.)
CNX_BIG_N, RN_BIG_N = GROUPED_ROWS + 1, GROUPED_ROWS // 4 + 1


def convnext_cases():
    """(id, ConvNextArch, proj2_bias, seed, stem_scale).  The last case is there for the LayerNorm eps alone: its stem convolution is 2^-10 of the seeded one,
    so the rows the stem LayerNorm sees have a variance of the order of eps, and 1e-5 against 1e-6 is a factor on every value behind it"""
    from marqo_amd.engine.archs import ConvNextArch
    rows = [(32, (1, 1, 2, 1), "linear", False, 1e-6), (32, (2, 1, 1, 1), "mlp", True, 1e-5), (32, (1, 1, 2, 1), "mlp", False, 1e-5),
            (64, (1, 1, 2, 1), "mlp", True, 1e-6), (64, (2, 1, 1, 1), "linear", False, 1e-5), (64, (2, 1, 1, 1), "mlp", False, 1e-6),
            (32, (1, 1, 2, 1), "linear", False, 1e-5)]
    out = []
    for i, (S, depths, head, b2, eps) in enumerate(rows):
        dim = i == len(rows) - 1
        cid = f"S{S}-d{''.join(map(str, depths))}-{head}{'+b2' if b2 else ''}-eps{eps:g}{'-dimstem' if dim else ''}"
        out.append((cid, ConvNextArch(S, depths, CNX_DIMS, eps, head, CNX_E), b2, 20 + i, 2.0 ** -10 if dim else 1.0))
    return out


def resnet_cases():
    """(id, ResNetArch, seed)"""
    from marqo_amd.engine.archs import ResNetArch
    out = []
    for S in (64, 96):
        for layers in ((1, 1, 1, 1), (2, 1, 2, 1)):
            for w in (16, 64, 80):
                out.append((f"S{S}-l{''.join(map(str, layers))}-w{w}", ResNetArch(S, layers, w, RN_E), 40 + len(out)))
    return out


ATTENTION_GAIN = 4.0


def convnext_sd(arch, proj2_bias: bool, seed: int, stem_scale: float = 1.0) -> Dict[str, Tensor]:
    from marqo_amd.engine import synthetic
    sd = synthetic.random_open_clip_state_dict(vision=arch, text=None, seed=seed)
    for k in ("visual.trunk.stem.0.weight", "visual.trunk.stem.0.bias"):
        sd[k] = sd[k] * stem_scale
    if proj2_bias:
        sd["visual.head.mlp.fc2.bias"] = 0.05 * torch.randn(arch.out_dim, generator=torch.Generator().manual_seed(seed + 500))
    return sd


def resnet_sd(arch, seed: int) -> Dict[str, Tensor]:
    """the seeded checkpoint with the attention pool's q_proj and k_proj weights times ATTENTION_GAIN: seeded projections give scores of a few hundredths,
    a near-uniform softmax whatever the temperature — a missing 64^-0.5 would change nothing.  With the gain the scores spread over a few units, as in
    synthetic.cross_encoder_state_dict"""
    from marqo_amd.engine import synthetic
    sd = synthetic.random_open_clip_state_dict(vision=arch, text=None, seed=seed)
    for k in ("visual.attnpool.q_proj.weight", "visual.attnpool.k_proj.weight"):
        sd[k] = sd[k] * ATTENTION_GAIN
    return sd


def images(n: int, S: int, seed: int) -> Tensor:
    """uint8 [n, S, S, 3]: natural-image statistics, every image another one; a batch of fewer images with the same seed is a prefix of a larger one"""
    from marqo_amd.engine import synthetic
    return synthetic.natural_images_u8(n, S, S, seed=seed)
