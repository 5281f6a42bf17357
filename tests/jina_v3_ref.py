"""Helpers of the Jina v3 tests (tests/test_jina_v3_host.py, tests/test_lora_gpu.py, tests/test_jina_v3_gpu.py).  Nothing here calls the library.

  - the tiny config TINY and seeded checkpoints built at test time: transformers' own JinaEmbeddingsV3Model(JinaEmbeddingsV3Config(...)) with working
    magnitudes (tiny_model), seeded task adapters of rank 4 on the six Linears and the token table (tiny_adapters), their PEFT directories
    (write_adapter_dir: adapter_config.json + adapter_model.safetensors in the documented key layout), the transformers model with W + scale B A merged
    into its nn.Linear / nn.Embedding weights (merged_model);
  - the LoRA kernels' float64 statement and rounding budgets (lora_down_ref, lora_up_ref);
  - exact / model: the float64 restatement of csrc/jina_v3.hip's block formula over a packed token stream with one task per sequence, in the manner of
    tests/nomic_bert_ref.py (Pass and row_ratio of tests/packed_text_ref.py are reused): `model` rounds to bf16 / fp32 exactly where the tower stores
    bf16 / fp32, `exact` rounds nothing.  `exact` is pinned to transformers' JinaEmbeddingsV3Model in float64 by tests/test_jina_v3_host.py.

Where `model` rounds (lora: the tower's adapter form, csrc/jina_v3.hip):  e = tok[ids] + type0 (+ fp32(T_emb) bf16(B_emb)^T, T_emb = fp32(scale A_emb[id]))
: fp32 ; n = LN_emb(e): x = fp32(n), h = bf16(n) ; qkv = bf16(h Wqkv^T + b), then bf16(qkv + T bf16(B)^T) with T = fp32(scale (h bf16(A)^T)) on adapter rows ;
(q | k) = bf16 once more behind the rotation ; p = bf16, un-normalised, for P V ; a = bf16 ; x = fp32(x + T_o B_o^T) on adapter rows ;
y = fp32(x + a Wo^T + b) ; n = LN_attn(y): x = fp32(n), h = bf16(n) ; pre = bf16(h W1^T + b) ; act = bf16(gelu(pre + T B^T)) — without adapters at all
(lora = None) act = bf16(gelu(h W1^T + b)), the GEMM's fused epilogue ; x = fp32(x + T_2 B_2^T) ; y = fp32(x + act W2^T + b) ; n = LN_mlp(y) ;
mean = fp32(sum / len) ; L2 = fp32(row / |row|)."""
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import torch

from tests import encoder_ref as E
from tests.jina_bert_ref import random_seqs      # noqa: F401
from tests.nomic_bert_ref import _attention, _rope_ang
from tests.packed_text_ref import Pass, row_ratio      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64
TASKS = ("retrieval.query", "retrieval.passage", "separation", "classification", "text-matching")
RANK = 4
ALPHA = 8.0
GELU_ABS = 7e-5            # |gelu_erf2(x) - gelu(x)|, the contract of csrc/common.h (tests/test_gemm_parity_gpu.py measures it)
GELU_SLOPE = 1.13          # max |gelu'(x)|

TINY = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=192, vocab_size=384, max_position_embeddings=2050,
            type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2)
PIN_LENS = [1, 7, 70]
MODULES = dict(q_proj="self_attn.q_proj", k_proj="self_attn.k_proj", v_proj="self_attn.v_proj", o_proj="self_attn.o_proj", fc1="mlp.fc1", fc2="mlp.fc2")


# ---- tiny checkpoints ---------------------------------------------------------------------------------------------------------------------------------
def tiny_model(seed: int = 0, gain: float = 0.6, **over):
    """transformers' JinaEmbeddingsV3Model on TINY (fp32, eval) with seeded working magnitudes in place of the 0.02 initialisation: LayerNorm weights
    1 + 0.1 N(0, 1), LayerNorm and Linear biases 0.1 N(0, 1), the token and type tables N(0, 1), Linear weights N(0, gain / sqrt(in)), q and k x 2; every
    Linear weight rounded to bf16 — what the tower stores"""
    from transformers import JinaEmbeddingsV3Config, JinaEmbeddingsV3Model
    m = JinaEmbeddingsV3Model(JinaEmbeddingsV3Config(**dict(TINY, **over)), add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(9000 + seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            rn = torch.randn(p.shape, generator=g)
            if "layernorm" in name.lower():
                p.copy_(1.0 + 0.1 * rn if name.endswith("weight") else 0.1 * rn)
            elif "embeddings." in name:
                p.copy_(rn)
            elif name.endswith("bias"):
                p.copy_(0.1 * rn)
            else:
                mul = 2.0 if (".q_proj." in name or ".k_proj." in name) else 1.0
                p.copy_((rn * (mul * gain / math.sqrt(p.shape[1]))).to(torch.bfloat16).float())
    return m


def tiny_adapters(cfg: dict, tasks: Sequence[str] = TASKS, rank: int = RANK, seed: int = 0) -> Dict[str, dict]:
    """{task: dict(r, alpha, tensors = {PEFT key: tensor})}: A ~ N(0, 1 / sqrt(in)), B ~ N(0, 0.5 / sqrt(r)) on every Linear, rounded to bf16 (what the tower
    stores), the embedding adapter A ~ N(0, 1), B ~ N(0, 0.3) — large enough that an adapter moves the embedding well past every bar"""
    W, F, V, nl = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_hidden_layers"]
    dims = dict(q_proj=(W, W), k_proj=(W, W), v_proj=(W, W), o_proj=(W, W), fc1=(F, W), fc2=(W, F))
    out = {}
    for i, task in enumerate(tasks):
        g = torch.Generator().manual_seed(31000 + 17 * seed + i)
        bf = lambda t: t.to(torch.bfloat16).float()
        t = {}
        for l in range(nl):
            for m, path in MODULES.items():
                o, k = dims[m]
                t[f"base_model.model.layers.{l}.{path}.lora_A.weight"] = bf(torch.randn(rank, k, generator=g) / math.sqrt(k))
                t[f"base_model.model.layers.{l}.{path}.lora_B.weight"] = bf(torch.randn(o, rank, generator=g) * (0.5 / math.sqrt(rank)))
        t["base_model.model.embeddings.word_embeddings.lora_embedding_A"] = torch.randn(rank, V, generator=g)
        t["base_model.model.embeddings.word_embeddings.lora_embedding_B"] = bf(torch.randn(W, rank, generator=g) * 0.3)
        out[task] = dict(r=rank, alpha=ALPHA, tensors=t)
    return out


def adapter_config(r: int = RANK, alpha: float = ALPHA, **over) -> dict:
    return dict(dict(peft_type="LORA", r=r, lora_alpha=alpha, target_modules=list(MODULES) + ["word_embeddings"], bias="none", use_dora=False,
                     use_rslora=False, lora_dropout=0.0, fan_in_fan_out=False, rank_pattern={}, alpha_pattern={}), **over)


def write_adapter_dir(directory, adapter: dict, prefix: str = "", **cfg_over) -> str:
    """adapter_config.json + adapter_model.safetensors; prefix "roberta.": the task-head classes' module path"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "adapter_config.json"), "w") as f:
        json.dump(adapter_config(adapter["r"], adapter["alpha"], **cfg_over), f)
    ren = lambda k: "base_model.model." + prefix + k[len("base_model.model."):]
    save_file({ren(k): v.contiguous() for k, v in adapter["tensors"].items()}, os.path.join(directory, "adapter_model.safetensors"))
    return str(directory)


def merged_model(m, adapter: Optional[dict], dtype=torch.float64):
    """a copy of the transformers model in `dtype` with W + scale B A merged into its nn.Linear weights and (scale B A)^T into its nn.Embedding table"""
    import copy
    mm = copy.deepcopy(m).to(dtype).eval()
    if adapter is None:
        return mm
    scale = adapter["alpha"] / adapter["r"]
    t = {k[len("base_model.model."):]: v.to(dtype) for k, v in adapter["tensors"].items()}
    with torch.no_grad():
        for name, p in mm.named_parameters():
            stem = name.rsplit(".", 1)[0]
            if name.endswith(".weight") and stem + ".lora_A.weight" in t:
                p += scale * (t[stem + ".lora_B.weight"] @ t[stem + ".lora_A.weight"])
            elif name == "embeddings.word_embeddings.weight":
                p += scale * (t[stem + ".lora_embedding_B"] @ t[stem + ".lora_embedding_A"]).T
    return mm


def write_tokenizer(directory, tokenizer):
    """tokenizer.json whose post-processor writes <s> ... </s> + tokenizer_config.json naming <pad>"""
    tokenizer.save(os.path.join(directory, "tokenizer.json"))
    with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
        json.dump({"bos_token": "<s>", "eos_token": "</s>", "cls_token": "<s>", "sep_token": "</s>", "pad_token": "<pad>", "unk_token": "<unk>"}, f)


def train_tokenizer(vocab_size: int = 384):
    """a small unigram tokenizer trained in memory with the XLM-RoBERTa specials at their ids (<s> 0, <pad> 1, </s> 2, <unk> 3) and the template <s> $A </s>"""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors, trainers
    tk = Tokenizer(models.Unigram())
    tk.pre_tokenizer = pre_tokenizers.Metaspace()
    corpus = ["hello world", "a search engine ranks documents for a query", "rotary positions turn every pair of dimensions by the token's index",
              "low rank adapters change a linear map by a thin product", "queries and passages share one batch"] * 4
    tk.train_from_iterator(corpus, trainers.UnigramTrainer(vocab_size=vocab_size, special_tokens=["<s>", "<pad>", "</s>", "<unk>"], unk_token="<unk>"))
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    return tk


# ---- the LoRA kernels in float64 --------------------------------------------------------------------------------------------------------------------
def seq_of_rows(lens: Sequence[int], device="cpu") -> Tensor:
    return torch.repeat_interleave(torch.arange(len(lens), device=device), torch.tensor(list(lens), device=device))


def lora_down_ref(x: Tensor, A: Tensor, scale: Tensor, row_task: Tensor):
    """x [rows, K], A [tasks, R, K] (bf16 values), scale [tasks], row_task int [rows] (-1: none) -> (T [rows, R] float64, budget [rows, R]).
    Budget: the products of two bf16 values are exact in fp32; the K of them are added in fp32 in an order the MFMA chooses — every one of the at most K
    roundings is at most 2^-24 of the sum of magnitudes — and the sum is multiplied by the scale (one more) and stored in fp32 (none):
    (K + 1) 2^-24 |scale| sum_k |x_k a_k|.  Rows without adapter: T = 0, budget 0."""
    rows, K = x.shape
    t = row_task.clamp(min=0).long()
    xa = x.double()[:, None, :] * A.double()[t]                    # [rows, R, K]
    sc = scale.double()[t][:, None]
    on = (row_task >= 0)[:, None].double()
    T = xa.sum(-1) * sc * on
    budget = (K + 1) * 2.0 ** -24 * sc.abs() * xa.abs().sum(-1) * on
    return T, budget


def lora_delta_ref(T: Tensor, B: Tensor, row_task: Tensor, nblocks: int):
    """T [rows, R] (fp32 values), B [tasks, N, r] (bf16 values) -> (delta [rows, N] float64, sum of |T_j b_j| [rows, N]); column block b reads T[:, b r : (b + 1) r]"""
    tasks, N, r = B.shape
    t = row_task.clamp(min=0).long()
    bc = N // nblocks
    Tb = T.double().reshape(T.shape[0], nblocks, r)[:, torch.arange(N, device=T.device) // bc, :]      # [rows, N, r]
    prod = Tb * B.double()[t]
    on = (row_task >= 0)[:, None].double()
    return prod.sum(-1) * on, prod.abs().sum(-1) * on


def lora_up_ref(T: Tensor, B: Tensor, row_task: Tensor, nblocks: int, out0: Tensor, mode: str, gelu: bool = False):
    """-> (out [rows, N] float64, budget).  r FMAs in fp32: r 2^-24 sum_j |T_j b_j| on the delta.  accumulate: + 2^-24 |out| (the fp32 add) ; write: nothing
    more ; in place: the fp32 add (2^-24 |pre|), the GELU's slope on that error plus its polynomial's contract (GELU_ABS), the bf16 store
    (half an ulp of 8 significant bits: 2^-8 |out|, the term of tests/attention_ref.py).
    Rows without adapter carry no delta error (accumulate / in place without GELU: out0 itself, budget 0)."""
    r = B.shape[2]
    delta, mag = lora_delta_ref(T, B, row_task, nblocks)
    db = r * 2.0 ** -24 * mag
    on = (row_task >= 0)[:, None].double()
    if mode == "accumulate":
        out = out0.double() + delta
        return out, (db + 2.0 ** -24 * out.abs()) * on
    if mode == "write":
        return delta, db
    pre = out0.double() + delta
    eb = (db + 2.0 ** -24 * pre.abs()) * on
    if gelu:
        out = E._act(pre, "gelu")
        return out, GELU_SLOPE * eb + GELU_ABS + 2.0 ** -8 * out.abs()
    return pre, (eb + 2.0 ** -8 * pre.abs()) * on


# ---- the float64 pass -------------------------------------------------------------------------------------------------------------------------------
_FORM = E.Form("jina_v3")


def operands(tensors: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """jina_v3_state_dict's fp32 tensors as the tower stores them, in float64: the weight matrices to bf16; the token table, biases and LayerNorm tensors fp32"""
    return {k: (E._w16(v) if v.dim() == 2 and k != "word_embeddings.weight" else E._f32(v)).to(device) for k, v in tensors.items()}


def lora_operands(lt: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """LoraSet.t as the tower stores it: everything bf16 but the scales and the transposed embedding A (fp32)"""
    return {k: (E._f32(v) if k in ("scale", "emb_a") else E._w16(v)).to(device) for k, v in lt.items()}


def _run(arch, tensors, lora, ids, lens, tasks, rounds, layers, hist) -> Pass:
    """lora: LoraSet.t or None; tasks: one adapter index per sequence (-1: none)"""
    dev = ids.device
    lens = [int(n) for n in lens]
    assert ids.dim() == 1 and ids.shape[0] == sum(lens) and min(lens) >= 1
    layers = arch.layers if layers is None else layers
    t = operands(tensors, dev)
    R = E._Round(_FORM if rounds else None)
    hist = hist if rounds else 0
    mm = lambda x, w: E._mm(x, w, hist)
    W, F, H, hd, eps = arch.width, arch.mlp_dim, arch.heads, arch.head_dim, arch.ln_eps
    rows = ids.shape[0]
    pos = E._positions(lens, dev)
    ang32 = pos.to(torch.float32)[:, None] * arch.inv_freq().to(dev)[None, :]
    rot = lambda part: _rope_ang(part.reshape(rows, H, hd), ang32).reshape(rows, W)
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt())
    ln = lambda y, name: E._ln(y, t[name + ".weight"], t[name + ".bias"], eps)
    if lora is not None:
        a = lora_operands(lora, dev)
        row_task = torch.as_tensor(list(tasks), device=dev)[seq_of_rows(lens, dev)]
        on = (row_task >= 0)[:, None].double()
        rt = row_task.clamp(min=0).long()
        sc = a["scale"][rt][:, None]

        def delta(x, name, nblocks=1):      # scale_t (x A_t^T) B_t^T per row, T stored in fp32
            A, B = a[name + "_a"][rt], a[name + "_b"][rt]                        # [rows, R, K], [rows, N, r]
            T = R.f(R.f(torch.einsum("mk,mrk->mr", x, A)) * sc)
            r, N = B.shape[2], B.shape[1]
            Tb = T.reshape(rows, nblocks, r)[:, torch.arange(N, device=dev) // (N // nblocks), :]
            return (Tb * B).sum(-1) * on
    e = t["word_embeddings.weight"][ids.long()] + t["type0"]
    if lora is not None and "emb_a" in a:
        T = R.f(a["emb_a"][rt, ids.long()] * sc)
        e = R.f(e) + (T[:, None, :] * a["emb_b"][rt]).sum(-1) * on
    n = ln(R.f(e), "emb_ln")
    x, h = R.f(n), R.b(n)
    streams: List[Tensor] = []
    for l in range(layers):
        p = f"layer.{l}."
        qkv = R.b(mm(h, t[p + "attn.qkv.weight"]) + t[p + "attn.qkv.bias"])
        if lora is not None:
            qkv = torch.where(on.bool(), R.b(qkv + delta(h, p + "qkv", 3)), qkv)
        q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
        q, k = R.b(rot(q)), R.b(rot(k))
        at = _attention(torch.cat([q, k, v], 1), lens, H, hd, scale, R)
        if lora is not None:
            x = R.f(x + delta(at, p + "out"))
        n = ln(R.f(x + mm(at, t[p + "attn.o.weight"]) + t[p + "attn.o.bias"]), p + "attn_ln")
        x, h = R.f(n), R.b(n)
        pre = mm(h, t[p + "mlp.fc1.weight"]) + t[p + "mlp.fc1.bias"]
        if lora is not None:
            act = R.b(E._act(R.b(pre) + delta(h, p + "fc1"), "gelu"))
            x = R.f(x + delta(act, p + "fc2"))
        else:
            act = R.b(E._act(pre, "gelu"))
        n = ln(R.f(x + mm(act, t[p + "mlp.fc2.weight"]) + t[p + "mlp.fc2.bias"]), p + "mlp_ln")
        x, h = R.f(n), R.b(n)
        streams.append(x)
    final = x                                     # no final norm
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    sums = torch.zeros(len(lens), W, dtype=F64, device=dev).index_add_(0, seq_of_rows(lens, dev), final)
    pools = {"mean": R.f(sums / torch.tensor(lens, dtype=F64, device=dev)[:, None]), "cls": final[first]}
    out = {}
    for name, prow in pools.items():
        out[(name, 0)] = prow
        out[(name, 1)] = R.f(prow / prow.norm(dim=-1, keepdim=True))
    return Pass(blocks=streams, final=final, pooled=out)


def exact(arch, tensors, lora, ids, lens, tasks, layers: Optional[int] = None) -> Pass:
    return _run(arch, tensors, lora, ids, lens, tasks, False, layers, 0)


def model(arch, tensors, lora, ids, lens, tasks, layers: Optional[int] = None, hist: int = 0) -> Pass:
    return _run(arch, tensors, lora, ids, lens, tasks, True, layers, hist)


_built: Dict[str, dict] = {}


def build() -> dict:
    """the seeded tiny checkpoint, built once per process: dict(model = transformers' module, cfg = its config as a dict, arch, sd, tensors =
    jina_v3_state_dict's output, adapters = tiny_adapters, lora = the LoraSet of all five)"""
    if not _built:
        from marqo_amd.engine import archs, jina_v3 as J
        m = tiny_model()
        cfg = dict(m.config.to_dict(), model_type="jina_embeddings_v3")
        arch = archs.bert_arch_from_hf_config(cfg)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        ads = tiny_adapters(cfg)
        _built.update(model=m, cfg=cfg, arch=arch, sd=sd, tensors=J.jina_v3_state_dict(arch, sd), adapters=ads, lora=lora_set(arch, ads))
    return _built


def lora_set(arch, adapters: Dict[str, dict]):
    """tiny_adapters' tensors through the loader's own parser, without the file system: what read_adapter returns, stacked"""
    import tempfile
    from marqo_amd.engine import jina_v3 as J
    with tempfile.TemporaryDirectory() as root:
        dirs = {task: write_adapter_dir(os.path.join(root, task), a) for task, a in adapters.items()}
        return J.load_adapters(arch, dirs)
