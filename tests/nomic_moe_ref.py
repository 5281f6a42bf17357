"""Helpers of the mixture-of-experts NomicBERT tests; nothing here calls the library.  The model is written from memory of the hub's
modeling_hf_nomic_bert.py (no copy was at hand).  route_ref / moe_mlp_ref: the kernels in float64 with per-element rounding budgets (derived as in
tests/jina_v3_ref.py::lora_down_ref and tests/gemm_ref.py: bf16 products are exact in fp32; a K-term fp32 sum is within (K + 1) 2^-24 sum |a b| in any
order; GELU_ABS / GELU_SLOPE; half a bf16 ulp 2^-8 |v| for the stored P).  exact / model: the whole pass; `model` rounds where the tower stores bf16 /
fp32 (routed block: logits and weights fp32 ; P = bf16(gelu(h W1[e]^T)) ; Y = fp32(w (P W2t[e]^T)) ; the combine's three adds in fp32 in the kernel's
order ; x = fp32(LN), h = bf16(LN)); attention and rotary code are tests/nomic_bert_ref.py's.  torch_fp32: the model in plain fp32 torch.  The tiny
checkpoint: W 128, 2 heads, F 192, E 4, k 2, 4 layers, 1 and 3 routed — the index rule (i + 1) % moe_every_n_layers == 0 is used HERE only."""
import math
from typing import Dict, List, Optional

import torch

from tests import encoder_ref as E
from tests.jina_v3_ref import GELU_ABS, GELU_SLOPE
from tests.nomic_bert_ref import _attention, _rope_ang, random_seqs, train_tokenizer, write_checkpoint_dir      # noqa: F401
from tests.packed_text_ref import Pass, row_ratio      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64
U = 2.0 ** -24
TINY = dict(n_embd=128, n_head=2, n_layer=4, n_inner=192, vocab_size=384, n_positions=2048, num_experts=4, moe_top_k=2, moe_every_n_layers=2)
TOWER_LENS = [1, 7, 64, 65, 130]
# A random router cannot keep every one of 2 x 267 deciding gaps 8 x above the bf16 model's logit error (the ratio does not depend on its scale): the tiny
# model gives token t a strong component along two of E orthonormal directions, AMP (D[a(t)] + D[b(t)] / 2), and router row e is ROUTER_GAIN D[e] plus a
# little noise.  The pair (a, b) walks all ordered pairs with the token id, so every expert serves rows of every sequence and a row's choice is its own.
AMP, ROUTER_GAIN = 16.0, 0.3


# ---- the kernels in float64 ---------------------------------------------------------------------------------------------------------------------------
def route_ref(x: Tensor, Wr: Tensor, k: int) -> dict:
    """x [rows, W], Wr [E, W] (fp32 values) -> logits, top_e [rows, k] (stable: the lower index wins a tie), top_w (softmax values, not renormalised),
    gap (k-th minus (k + 1)-th largest logit; inf when k == E), bound = (W + 1) 2^-24 max_e sum |x w| (the fp32 accumulation bound of a row's logits) and
    w_budget: a logit error d moves p_e by at most 2 d p_e <= 2 d; expf (2 ulp each), the E-term sum and the division add (E + 8) 2^-23 p."""
    x, Wr = x.double(), Wr.double()
    E_, W = Wr.shape
    logits = x @ Wr.T
    order = torch.sort(-logits, dim=-1, stable=True).indices
    top_e = order[:, :k]
    p = torch.softmax(logits, -1)
    srt = torch.gather(logits, 1, order)
    gap = srt[:, k - 1] - srt[:, k] if k < E_ else torch.full_like(srt[:, 0], float("inf"))
    bound = (W + 1) * U * (x.abs() @ Wr.abs().T).amax(-1)
    top_w = torch.gather(p, 1, top_e)
    return dict(logits=logits, top_e=top_e, top_w=top_w, gap=gap, bound=bound, w_budget=2 * bound[:, None] + (E_ + 8) * 2 * U * top_w)


def moe_mlp_ref(h: Tensor, top_e: Tensor, top_w: Tensor, w1: Tensor, w2t: Tensor):
    """h [rows, W] (bf16 values), top_e / top_w [rows, k], w1 [E, F, W], w2t [E, W, F] (bf16 values) -> (Y [rows, k, W] float64, budget [rows, k, W]):
    Y[r, j] = w (gelu(h W1[e]^T) W2t[e]^T) with nothing rounded.  Budget per element: u = h W1^T is off by bu = (W + 1) 2^-24 sum |h w1|; the GELU by
    bg = GELU_SLOPE bu + GELU_ABS; the bf16 store of P by 2^-8 (|g| + bg): bp; the second sum by sum_f bp |w2| + (F + 1) 2^-24 sum_f (|g| + bp) |w2|; the
    product with w and the fp32 store by 2^-24 |Y| each."""
    h, tw = h.double(), top_w.double()
    W, F = h.shape[1], w1.shape[1]
    rows, k = top_e.shape
    y, by = torch.zeros(rows * k, w2t.shape[1], dtype=F64), torch.zeros(rows * k, w2t.shape[1], dtype=F64)
    flat = top_e.flatten().long()
    for e in flat.unique().tolist():            # expert by expert: the entries i = row k + j it serves
        i = (flat == e).nonzero()[:, 0]
        a1, a2, he = w1[e].double(), w2t[e].double(), h[i // k]
        g = E._act(he @ a1.T, "gelu")
        bp = GELU_SLOPE * (W + 1) * U * (he.abs() @ a1.abs().T) + GELU_ABS
        bp = bp + 2.0 ** -8 * (g.abs() + bp)
        y[i] = g @ a2.T
        by[i] = bp @ a2.abs().T + (F + 1) * U * ((g.abs() + bp) @ a2.abs().T)
    Y = tw[..., None] * y.reshape(rows, k, -1)
    return Y, tw.abs()[..., None] * by.reshape(rows, k, -1) + 2 * U * Y.abs()


# ---- the tiny checkpoint ---------------------------------------------------------------------------------------------------------------------------------
def hub_config(**over) -> dict:
    """config.json in the hub's GPT-2-style keys, as nomic-embed-text-v2-moe's is remembered"""
    return dict(dict(TINY, model_type="nomic_bert", architectures=["NomicBertModel"], activation_function="gelu", type_vocab_size=1,
                     layer_norm_epsilon=1e-5, rotary_emb_base=10000, rotary_emb_fraction=1.0, rotary_emb_interleaved=False, rotary_scaling_factor=None,
                     qkv_proj_bias=True, mlp_fc1_bias=True, mlp_fc2_bias=True, prenorm=False, use_rms_norm=False, moe_normalize_expert_weights=False,
                     expert_choice_router=False), **over)


def tiny_state_dict(seed: int = 0, gain: float = 0.6) -> Dict[str, Tensor]:
    """seeded working magnitudes under the hub's tensor names (tests/nomic_bert_ref.py::tiny_model's rules): LayerNorm 1 + 0.1 N / 0.1 N, tables N(0, 1),
    Linear and expert matrices N(0, gain / sqrt(in)) rounded to bf16, q and k rows x 2, biases 0.1 N; the token table and the routers carry the
    directions D (see AMP above), the routers in fp32"""
    W, F, E_, L, V = TINY["n_embd"], TINY["n_inner"], TINY["num_experts"], TINY["n_layer"], TINY["vocab_size"]
    g = torch.Generator().manual_seed(9000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    lin = lambda n, k: (rn(n, k) * (gain / math.sqrt(k))).to(torch.bfloat16).float()
    D = torch.linalg.qr(rn(W, E_)).Q.T.contiguous()                      # [E, W] orthonormal rows
    tok = torch.arange(V)
    a = tok % E_
    b = (a + 1 + (tok // E_) % (E_ - 1)) % E_
    sd = {"embeddings.word_embeddings.weight": rn(V, W) + AMP * (D[a] + 0.5 * D[b]), "embeddings.token_type_embeddings.weight": rn(1, W), "emb_ln.weight": 1 + 0.1 * rn(W),
          "emb_ln.bias": 0.1 * rn(W)}
    for l in range(L):
        p = f"encoder.layers.{l}."
        qkv = lin(3 * W, W)
        qkv[:2 * W] = (qkv[:2 * W] * 2).to(torch.bfloat16).float()
        sd.update({p + "attn.Wqkv.weight": qkv, p + "attn.Wqkv.bias": 0.1 * rn(3 * W), p + "attn.out_proj.weight": lin(W, W),
                   p + "attn.out_proj.bias": 0.1 * rn(W)})
        for n in ("norm1", "norm2"):
            sd.update({p + n + ".weight": 1 + 0.1 * rn(W), p + n + ".bias": 0.1 * rn(W)})
        if (l + 1) % TINY["moe_every_n_layers"] == 0:
            sd.update({p + "mlp.router.layer.weight": ROUTER_GAIN * D + rn(E_, W) * (0.1 / math.sqrt(W)), p + "mlp.experts.mlp.w1": lin(E_ * F, W),
                       p + "mlp.experts.mlp.w2": (rn(E_ * F, W) * (gain / math.sqrt(F))).to(torch.bfloat16).float(), p + "mlp.experts.bias": 0.1 * rn(W)})
        else:
            sd.update({p + "mlp.fc1.weight": lin(F, W), p + "mlp.fc1.bias": 0.1 * rn(F), p + "mlp.fc2.weight": lin(W, F), p + "mlp.fc2.bias": 0.1 * rn(W)})
    return sd


_built: Dict[str, dict] = {}


def build() -> dict:
    """dict(cfg, arch, sd (hub names), tensors = nomic_moe_state_dict's output, seqs), once per process"""
    if not _built:
        from marqo_amd.engine import archs, tower_weights as TW
        cfg, sd = hub_config(), tiny_state_dict()
        arch = archs.bert_arch_from_hf_config(cfg)
        _built.update(cfg=cfg, arch=arch, sd=sd, tensors=TW.nomic_moe_state_dict(arch, sd), seqs=random_seqs(TOWER_LENS, cfg["vocab_size"], seed=3))
    return _built


# ---- the float64 pass -------------------------------------------------------------------------------------------------------------------------------
_FORM = E.Form("nomic_moe")


def operands(tensors: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """nomic_moe_state_dict's tensors as the tower stores them, in float64: matrices and expert stacks to bf16; the token table, the ROUTER, biases and
    LayerNorm tensors fp32"""
    keep = lambda k, v: v.dim() < 2 or k == "word_embeddings.weight" or k.endswith("moe.router.weight")
    return {k: (E._f32(v) if keep(k, v) else E._w16(v)).to(device) for k, v in tensors.items()}


def _run(arch, tensors, ids, lens, rounds, layers, hist, rec) -> Pass:
    dev = ids.device
    lens = [int(n) for n in lens]
    assert ids.dim() == 1 and ids.shape[0] == sum(lens) and min(lens) >= 1
    layers = arch.layers if layers is None else layers
    t = operands(tensors, dev)
    R = E._Round(_FORM if rounds else None)
    mm = lambda x, w: E._mm(x, w, hist if rounds else 0)
    W, H, hd, eps, k = arch.width, arch.heads, arch.head_dim, arch.ln_eps, arch.top_k
    rows = ids.shape[0]
    ang32 = E._positions(lens, dev).to(torch.float32)[:, None] * arch.inv_freq().to(dev)[None, :]
    rot = lambda part: _rope_ang(part.reshape(rows, H, hd), ang32).reshape(rows, W)
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt())
    ln = lambda y, name: E._ln(y, t[name + ".weight"], t[name + ".bias"], eps)
    n = ln(R.f(t["word_embeddings.weight"][ids.long()] + t["type0"]), "emb_ln")
    x, h = R.f(n), R.b(n)
    streams: List[Tensor] = []
    for l in range(layers):
        p = f"layer.{l}."
        qkv = R.b(mm(h, t[p + "attn.qkv.weight"]) + t[p + "attn.qkv.bias"])
        q, kk, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
        at = _attention(torch.cat([R.b(rot(q)), R.b(rot(kk)), v], 1), lens, H, hd, scale, R)
        n = ln(R.f(x + mm(at, t[p + "attn.o.weight"]) + t[p + "attn.o.bias"]), p + "attn_ln")
        x, h = R.f(n), R.b(n)
        if p + "moe.router.weight" in t:
            r = route_ref(x, t[p + "moe.router.weight"], k)
            if rec is not None:
                rec[l] = r
            y = x
            for j in range(k):
                e = r["top_e"][:, j]
                P = R.b(E._act(torch.einsum("rw,rfw->rf", h, t[p + "moe.w1"][e]), "gelu"))
                y = R.f(y + R.f(R.f(r["top_w"][:, j, None]) * torch.einsum("rf,rwf->rw", P, t[p + "moe.w2t"][e])))
            n = ln(R.f(y + t[p + "moe.bias"]), p + "mlp_ln")
        else:
            act = R.b(E._act(mm(h, t[p + "mlp.fc1.weight"]) + t[p + "mlp.fc1.bias"], "gelu"))
            n = ln(R.f(x + mm(act, t[p + "mlp.fc2.weight"]) + t[p + "mlp.fc2.bias"]), p + "mlp_ln")
        x, h = R.f(n), R.b(n)
        streams.append(x)
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    seq_of = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.tensor(lens, device=dev))
    sums = torch.zeros(len(lens), W, dtype=F64, device=dev).index_add_(0, seq_of, x)
    pools = {"mean": R.f(sums / torch.tensor(lens, dtype=F64, device=dev)[:, None]), "cls": x[first]}
    out = {}
    for name, prow in pools.items():
        out[(name, 0)] = prow
        out[(name, 1)] = R.f(prow / prow.norm(dim=-1, keepdim=True))
    return Pass(blocks=streams, final=x, pooled=out)


def exact(arch, tensors, ids, lens, layers: Optional[int] = None, rec: Optional[dict] = None) -> Pass:
    return _run(arch, tensors, ids, lens, False, layers, 0, rec)


def model(arch, tensors, ids, lens, layers: Optional[int] = None, hist: int = 0, rec: Optional[dict] = None) -> Pass:
    return _run(arch, tensors, ids, lens, True, layers, hist, rec)


def torch_fp32(cfg: dict, sd: Dict[str, Tensor], ids: Tensor, pooling: str, normalize: bool) -> Tensor:
    """one sequence through the model in plain fp32 torch (hub names, no packing, no engine code) -> [W]"""
    F = torch.nn.functional
    W, H, k, eps = cfg["n_embd"], cfg["n_head"], cfg["moe_top_k"], cfg["layer_norm_epsilon"]
    hd, T = W // H, ids.shape[0]
    inv = 1.0 / (float(cfg["rotary_emb_base"]) ** (torch.arange(0, hd, 2).float() / hd))
    ang = torch.arange(T).float()[:, None] * inv[None, :]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1)[None], torch.cat([ang.sin(), ang.sin()], -1)[None]
    half = lambda z: torch.cat([-z[..., hd // 2:], z[..., :hd // 2]], -1)
    x = F.layer_norm(sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.token_type_embeddings.weight"][0], (W,), sd["emb_ln.weight"],
                     sd["emb_ln.bias"], eps)
    for l in range(cfg["n_layer"]):
        p = f"encoder.layers.{l}."
        q, kk, v = (F.linear(x, sd[p + "attn.Wqkv.weight"], sd[p + "attn.Wqkv.bias"]).reshape(T, 3, H, hd).permute(1, 2, 0, 3))
        q, kk = q * cos + half(q) * sin, kk * cos + half(kk) * sin
        a = (torch.softmax(q @ kk.transpose(1, 2) / math.sqrt(hd), -1) @ v).transpose(0, 1).reshape(T, W)
        x = F.layer_norm(x + F.linear(a, sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"]), (W,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        if p + "mlp.router.layer.weight" in sd:
            E_ = sd[p + "mlp.router.layer.weight"].shape[0]
            w1, w2 = sd[p + "mlp.experts.mlp.w1"].reshape(E_, -1, W), sd[p + "mlp.experts.mlp.w2"].reshape(E_, -1, W)
            tw, te = torch.softmax(x @ sd[p + "mlp.router.layer.weight"].T, -1).topk(k, -1)
            y = sum(tw[:, j, None] * torch.einsum("tf,tfw->tw", F.gelu(torch.einsum("tw,tfw->tf", x, w1[te[:, j]])), w2[te[:, j]]) for j in range(k))
            y = y + sd[p + "mlp.experts.bias"]
        else:
            y = F.linear(F.gelu(F.linear(x, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        x = F.layer_norm(x + y, (W,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    v = x.mean(0) if pooling == "mean" else x[0]
    return v / v.norm() if normalize else v
