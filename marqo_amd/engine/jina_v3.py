"""Jina v3 text tower: jina-embeddings-v3 in transformers' own form (config.json: model_type "jina_embeddings_v3", JinaEmbeddingsV3Model tensor names) with
its task LoRA adapters -> HBM layout -> one mq_encode_jina_v3 call per batch of packed sequences (csrc/jina_v3.hip; the LoRA kernels: csrc/lora.hip).

bf16 GEMM operands, fp32 residual stream, 64-wide heads, sequences up to 8192 tokens.  The adapters are NOT merged into the weights: every sequence of a
batch names its own task (or none) and the kernels add the rank-r correction per row, so queries and passages share a call.  The block semantics and the
LoRA delta are pinned to transformers' JinaEmbeddingsV3Model in float64 (tests/test_jina_v3_host.py).

Adapter directories are PEFT's layout, written from its documented format — NOT verified against a real hub file (`peft` is not a dependency):
adapter_config.json {r, lora_alpha, target_modules, bias, use_rslora, use_dora} + adapter_model.safetensors with
`base_model.model.[roberta.]<module>.lora_A.weight` [r, in], `.lora_B.weight` [out, r] for the Linears q_proj / k_proj / v_proj / o_proj / fc1 / fc2 and
`base_model.model.[roberta.]embeddings.word_embeddings.lora_embedding_A` [r, vocab], `.lora_embedding_B` [W, r]."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import JinaV3Arch
from marqo_amd.engine.towers import _PackedTextTower, _check_precision, _ids_and_lengths, _large_call, _need

Tensor = torch.Tensor
MAX_RANK = 16
LINEARS = ("q_proj", "k_proj", "v_proj", "o_proj", "fc1", "fc2")
EMBEDDING = "word_embeddings"
_LINEAR_KEY = re.compile(r"^layers\.(\d+)\.(?:self_attn\.(q_proj|k_proj|v_proj|o_proj)|mlp\.(fc1|fc2))\.lora_([AB])\.weight$")
_EMBED_KEY = re.compile(r"^embeddings\.word_embeddings\.lora_embedding_([AB])$")


def jina_v3_state_dict(arch: JinaV3Arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """JinaEmbeddingsV3Model tensors (with or without the task-head classes' `roberta.` prefix) -> the fp32 tensors the tower hands to the kernels, from
    transformers' module names (embeddings.LayerNorm, layers.l.self_attn.{q,k,v,o}_proj, post_attention_layernorm, post_mlp_layernorm) or the names
    `save_pretrained` leaves on disk, the "jina_embeddings_v3" entry of transformers' conversion_mapping.py read from right to left (emb_ln,
    encoder.layers.l.mixer.Wqkv [3 W, W] = q, k, v along dim 0, mixer.out_proj, norm1, norm2).  Per block l: `layer.l.attn.qkv.weight` [3 W, W] / `.bias` [3 W] = rows q | k | v.  `type0` is row 0 of the token-type table.  Ignored: pooler, LM-head and
    classifier tensors, buffers.  Refused by name: a missing or mis-shaped tensor."""
    if "embeddings.word_embeddings.weight" not in sd and "roberta.embeddings.word_embeddings.weight" in sd:
        sd = {k[len("roberta."):]: v for k, v in sd.items() if k.startswith("roberta.")}
    disk = any(k.startswith("encoder.layers.") for k in sd) or "emb_ln.weight" in sd
    W, F = arch.width, arch.mlp_dim
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    emb_ln = "emb_ln" if disk else "embeddings.LayerNorm"
    out = {"word_embeddings.weight": f32("embeddings.word_embeddings.weight", (arch.vocab, W)),
           "type0": f32("embeddings.token_type_embeddings.weight", (arch.type_vocab, W))[0].contiguous(),
           "emb_ln.weight": f32(emb_ln + ".weight", (W,)), "emb_ln.bias": f32(emb_ln + ".bias", (W,))}
    for l in range(arch.layers):
        p = f"layer.{l}."
        if disk:
            src = f"encoder.layers.{l}."
            o, ln1, ln2 = src + "mixer.out_proj", src + "norm1", src + "norm2"
            out[p + "attn.qkv.weight"], out[p + "attn.qkv.bias"] = f32(src + "mixer.Wqkv.weight", (3 * W, W)), f32(src + "mixer.Wqkv.bias", (3 * W,))
        else:
            src = f"layers.{l}."
            o, ln1, ln2 = src + "self_attn.o_proj", src + "post_attention_layernorm", src + "post_mlp_layernorm"
            out[p + "attn.qkv.weight"] = torch.cat([f32(src + f"self_attn.{c}_proj.weight", (W, W)) for c in "qkv"], 0)
            out[p + "attn.qkv.bias"] = torch.cat([f32(src + f"self_attn.{c}_proj.bias", (W,)) for c in "qkv"], 0)
        out[p + "attn.o.weight"], out[p + "attn.o.bias"] = f32(o + ".weight", (W, W)), f32(o + ".bias", (W,))
        out[p + "attn_ln.weight"], out[p + "attn_ln.bias"] = f32(ln1 + ".weight", (W,)), f32(ln1 + ".bias", (W,))
        out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = f32(src + "mlp.fc1.weight", (F, W)), f32(src + "mlp.fc1.bias", (F,))
        out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = f32(src + "mlp.fc2.weight", (W, F)), f32(src + "mlp.fc2.bias", (W,))
        out[p + "mlp_ln.weight"], out[p + "mlp_ln.bias"] = f32(ln2 + ".weight", (W,)), f32(ln2 + ".bias", (W,))
    return out


# ---- adapters ------------------------------------------------------------------------------------------------------------------------------------------
def find_adapter_dirs(directory: str) -> Dict[str, str]:
    """every sub-directory of a checkpoint that holds adapter_config.json + adapter_model.safetensors -> {its name: its path}"""
    out = {}
    for name in sorted(os.listdir(directory)):
        d = os.path.join(directory, name)
        if os.path.isfile(os.path.join(d, "adapter_config.json")) and os.path.isfile(os.path.join(d, "adapter_model.safetensors")):
            out[name] = d
    return out


def read_adapter(task: str, directory: str, arch: JinaV3Arch) -> dict:
    """One PEFT adapter directory -> dict(rank, scale, linear = {(layer, module): (A [r, in], B [out, r])}, embedding = (A [r, vocab], B [W, r]) or None), fp32.
    ValueError, with the adapter's name and the reason: a target module outside the six Linears and the word embedding, bias other than "none", DoRA, a
    rank above 16, ranks that differ across modules (rank_pattern / alpha_pattern, or a tensor whose rank is not the config's), a missing half, a
    mis-shaped or unexpected tensor."""
    from safetensors.torch import load_file
    what = f"LoRA adapter {task!r} ({directory})"
    try:
        with open(os.path.join(directory, "adapter_config.json")) as f:
            ac = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"{what}: cannot read adapter_config.json: {e}") from e
    if str(ac.get("peft_type", "LORA")).upper() != "LORA":
        raise ValueError(f"{what}: peft_type={ac.get('peft_type')} is not served (LORA only)")
    if ac.get("use_dora", False):
        raise ValueError(f"{what}: use_dora is set: DoRA adapters are not served")
    if ac.get("bias", "none") != "none":
        raise ValueError(f"{what}: bias={ac.get('bias')!r} is not served (bias must be 'none')")
    if ac.get("rank_pattern") or ac.get("alpha_pattern"):
        raise ValueError(f"{what}: rank_pattern / alpha_pattern give ranks that differ across modules, which is not served (one rank and one scale per adapter)")
    targets = ac.get("target_modules")
    targets = [targets] if isinstance(targets, str) else list(targets or [])
    bad = [t for t in targets if t.rsplit(".", 1)[-1] not in LINEARS + (EMBEDDING,)]
    if bad:
        raise ValueError(f"{what}: target_modules {bad} are outside the six Linears ({', '.join(LINEARS)}) and {EMBEDDING}")
    r = ac.get("r")
    if not isinstance(r, int) or r < 1:
        raise ValueError(f"{what}: r={r!r} must be a positive integer")
    if r > MAX_RANK:
        raise ValueError(f"{what}: rank r={r} is above {MAX_RANK}, the largest rank the LoRA kernels run")
    alpha = float(ac.get("lora_alpha", r))
    scale = alpha / math.sqrt(r) if ac.get("use_rslora", False) else alpha / r
    W, F = arch.width, arch.mlp_dim
    dims = dict(q_proj=(W, W), k_proj=(W, W), v_proj=(W, W), o_proj=(W, W), fc1=(F, W), fc2=(W, F))      # (out, in)
    halves: Dict[tuple, Dict[str, Tensor]] = {}
    emb: Dict[str, Tensor] = {}
    for key, t in load_file(os.path.join(directory, "adapter_model.safetensors")).items():
        k = key[len("base_model.model."):] if key.startswith("base_model.model.") else key
        k = k[len("roberta."):] if k.startswith("roberta.") else k
        m = _LINEAR_KEY.match(k)
        if m:
            layer, module, half = int(m.group(1)), m.group(2) or m.group(3), m.group(4)
            if layer >= arch.layers:
                raise ValueError(f"{what}: tensor '{key}' names layer {layer} of a {arch.layers}-layer model")
            out_dim, in_dim = dims[module]
            want = (r, in_dim) if half == "A" else (out_dim, r)
            if tuple(t.shape) != want:
                if t.dim() == 2 and (t.shape[1] == in_dim if half == "A" else t.shape[0] == out_dim):
                    raise ValueError(f"{what}: tensor '{key}' has rank {t.shape[0] if half == 'A' else t.shape[1]} where adapter_config.json says r={r}: "
                                     f"ranks that differ across modules are not served")
                raise ValueError(f"{what}: tensor '{key}' has shape {tuple(t.shape)}, expected {want}")
            halves.setdefault((layer, module), {})[half] = t.detach().to(torch.float32)
            continue
        m = _EMBED_KEY.match(k)
        if m:
            want = (r, arch.vocab) if m.group(1) == "A" else (W, r)
            if tuple(t.shape) != want:
                if t.dim() == 2 and (t.shape[1] == arch.vocab if m.group(1) == "A" else t.shape[0] == W):
                    raise ValueError(f"{what}: tensor '{key}' has rank {t.shape[0] if m.group(1) == 'A' else t.shape[1]} where adapter_config.json says "
                                     f"r={r}: ranks that differ across modules are not served")
                raise ValueError(f"{what}: tensor '{key}' has shape {tuple(t.shape)}, expected {want}")
            emb[m.group(1)] = t.detach().to(torch.float32)
            continue
        raise ValueError(f"{what}: tensor '{key}' is unexpected (adapters of the six Linears and of {EMBEDDING} only; a trained bias or a DoRA magnitude is "
                         f"not served)")
    for (layer, module), h in halves.items():
        if set(h) != {"A", "B"}:
            raise ValueError(f"{what}: layers.{layer} {module} has lora_{'A' if 'A' in h else 'B'} without its other half")
    if emb and set(emb) != {"A", "B"}:
        raise ValueError(f"{what}: {EMBEDDING} has one of lora_embedding_A / lora_embedding_B without the other")
    if not halves and not emb:
        raise ValueError(f"{what}: adapter_model.safetensors holds no LoRA tensor")
    return dict(rank=r, scale=scale, linear={k: (h["A"], h["B"]) for k, h in halves.items()}, embedding=(emb["A"], emb["B"]) if emb else None)


class LoraSet:
    """The adapters of a checkpoint, stacked over tasks in the layouts of mq_jina_v3_lora (include/marqo_hip.h), fp32 on the host: `names` (task t's name),
    `rank` (the largest rank, padded up to a multiple of 4 with zeros — exact: a zero row of A and a zero column of B add nothing), `t` = {"scale"
    [tasks], "emb_a" [tasks, vocab, r] / "emb_b" [tasks, W, r] (absent when no task adapts the token table), "layer.l.qkv_a" [tasks, 3 r, W],
    "layer.l.qkv_b" [tasks, 3 W, r], "layer.l.out_a / fc1_a / fc2_a" [tasks, r, in], "layer.l.out_b / fc1_b / fc2_b" [tasks, out, r]}.  A Linear that a task
    does not adapt carries zeros for it."""

    def __init__(self, arch: JinaV3Arch, adapters: Dict[str, dict]):
        if not adapters:
            raise ValueError("no LoRA adapter given")
        self.names = list(adapters)
        nt = len(self.names)
        r = self.rank = -(-max(a["rank"] for a in adapters.values()) // 4) * 4
        W, F = arch.width, arch.mlp_dim
        t = self.t = {"scale": torch.tensor([adapters[n]["scale"] for n in self.names], dtype=torch.float32)}
        if any(a["embedding"] is not None for a in adapters.values()):
            t["emb_a"], t["emb_b"] = torch.zeros(nt, arch.vocab, r), torch.zeros(nt, W, r)
        dims = dict(out=("o_proj", W, W), fc1=("fc1", F, W), fc2=("fc2", W, F))
        for l in range(arch.layers):
            t[f"layer.{l}.qkv_a"], t[f"layer.{l}.qkv_b"] = torch.zeros(nt, 3 * r, W), torch.zeros(nt, 3 * W, r)
            for short, (_, out_dim, in_dim) in dims.items():
                t[f"layer.{l}.{short}_a"], t[f"layer.{l}.{short}_b"] = torch.zeros(nt, r, in_dim), torch.zeros(nt, out_dim, r)
        for i, n in enumerate(self.names):
            a = adapters[n]
            ra = a["rank"]
            if a["embedding"] is not None:
                t["emb_a"][i, :, :ra], t["emb_b"][i, :, :ra] = a["embedding"][0].t(), a["embedding"][1]
            for (l, module), (A, B) in a["linear"].items():
                if module in ("q_proj", "k_proj", "v_proj"):
                    b = "qkv".index(module[0])
                    t[f"layer.{l}.qkv_a"][i, b * r:b * r + ra], t[f"layer.{l}.qkv_b"][i, b * W:(b + 1) * W, :ra] = A, B
                else:
                    short = "out" if module == "o_proj" else module
                    t[f"layer.{l}.{short}_a"][i, :ra], t[f"layer.{l}.{short}_b"][i, :, :ra] = A, B

    def task_id(self, name: Optional[str]) -> int:
        if name is None:
            return -1
        if name not in self.names:
            raise ValueError(f"unknown LoRA task {name!r}: this checkpoint has {self.names}")
        return self.names.index(name)


def load_adapters(arch: JinaV3Arch, dirs: Dict[str, str]) -> Optional[LoraSet]:
    """{task name: adapter directory} -> LoraSet (None for an empty dict)"""
    return LoraSet(arch, {task: read_adapter(task, d, arch) for task, d in dirs.items()}) if dirs else None


class JinaV3Tower(_PackedTextTower):
    """Jina v3 encoder + per-sequence task adapters + mean / CLS pooling (+ L2).  `encode(ids, attention_mask, tasks=[...])` names one task (or None) per
    sequence; `encode_ids` (the loaders' interface) runs every sequence on `default_task`."""
    family = "jina_v3"

    def __init__(self, arch: JinaV3Arch, sd: Dict[str, Tensor], device: str, pooling: str = "mean", precision: str = "bf16",
                 adapters: Optional[LoraSet] = None, default_task: Optional[str] = None):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the Jina v3 tower runs on bf16 operands only (its rotary blocks and LoRA corrections have no e4m3 kernels), "
                                               f"got precision {precision!r}")
        if arch.head_dim != 64 or arch.width != arch.heads * 64:
            raise ValueError(f"the Jina v3 tower runs 64-wide attention heads only (hidden_size {arch.width}, num_attention_heads {arch.heads})")
        if arch.width > 2048:
            raise ValueError(f"the Jina v3 tower runs widths up to 2048 (hidden_size {arch.width})")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        self.precision, self.arch, self.pooling, self.adapters = precision, arch, pooling, adapters
        self._fp8 = None
        if default_task is not None and (adapters is None or default_task not in adapters.names):
            raise ValueError(f"unknown LoRA task {default_task!r}: this checkpoint has {adapters.names if adapters else 'no adapters'}")
        self.default_task = default_task
        h = self._h
        t = jina_v3_state_dict(arch, sd)
        self._layers = (L.JinaV3Layer * arch.layers)()
        for l in range(arch.layers):
            p = f"layer.{l}."
            self._layers[l] = L.JinaV3Layer(qkv_w=h.bf16(t[p + "attn.qkv.weight"]), qkv_b=h.f32(t[p + "attn.qkv.bias"]),
                                            out_w=h.bf16(t[p + "attn.o.weight"]), out_b=h.f32(t[p + "attn.o.bias"]),
                                            attn_ln_g=h.f32(t[p + "attn_ln.weight"]), attn_ln_b=h.f32(t[p + "attn_ln.bias"]),
                                            fc1_w=h.bf16(t[p + "mlp.fc1.weight"]), fc1_b=h.f32(t[p + "mlp.fc1.bias"]),
                                            fc2_w=h.bf16(t[p + "mlp.fc2.weight"]), fc2_b=h.f32(t[p + "mlp.fc2.bias"]),
                                            mlp_ln_g=h.f32(t[p + "mlp_ln.weight"]), mlp_ln_b=h.f32(t[p + "mlp_ln.bias"]))
        self.w = L.JinaV3Weights(tok_emb=h.f32(t["word_embeddings.weight"]), type0=h.f32(t["type0"]), emb_ln_g=h.f32(t["emb_ln.weight"]),
                                 emb_ln_b=h.f32(t["emb_ln.bias"]), d_inv_freq=h.f32(arch.inv_freq()), layers=self._layers)
        self.cfg = L.JinaV3Cfg(width=arch.width, layers=arch.layers, heads=arch.heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim, vocab=arch.vocab,
                               max_pos=arch.max_pos, pool=L.MQ_POOL_CLS if pooling == "cls" else L.MQ_POOL_MEAN, ln_eps=arch.ln_eps, reserved=0)
        self.lora = None
        if adapters is not None:
            a = adapters.t
            self._lora_layers = (L.JinaV3LoraLayer * arch.layers)()
            for l in range(arch.layers):
                self._lora_layers[l] = L.JinaV3LoraLayer(**{f"{m}_{half}": h.bf16(a[f"layer.{l}.{m}_{half}"]) for m in ("qkv", "out", "fc1", "fc2")
                                                            for half in "ab"})
            self.lora = L.JinaV3Lora(tasks=len(adapters.names), rank=adapters.rank, d_scale=h.f32(a["scale"]),
                                     emb_a=h.f32(a["emb_a"]) if "emb_a" in a else None, emb_b=h.bf16(a["emb_b"]) if "emb_b" in a else None,
                                     layers=self._lora_layers)

    def task_ids(self, tasks: Optional[Sequence[Optional[str]]], n: int) -> np.ndarray:
        """one task name (or None: no adapter) per sequence -> int32 [n] of adapter indices, -1 for none; ValueError for an unknown name"""
        if tasks is None:
            tasks = [self.default_task] * n
        if len(tasks) != n:
            raise ValueError(f"tasks names {len(tasks)} sequences, the batch has {n}")
        if self.adapters is None:
            if any(t is not None for t in tasks):
                raise ValueError(f"unknown LoRA task {next(t for t in tasks if t is not None)!r}: this checkpoint has no adapters")
            return np.full(n, -1, dtype=np.int32)
        return np.asarray([self.adapters.task_id(t) for t in tasks], dtype=np.int32)

    def encode(self, ids: Tensor, attention_mask: Tensor, tasks: Optional[Sequence[Optional[str]]] = None, normalize: bool = True) -> Tensor:
        """ids / attention_mask: int [n, S], right-padded; tasks: one adapter name or None per sequence (default: `default_task` for all) -> fp32
        [n, width] on the device.  Sequences of different tasks run in the same launch sequence."""
        ids_h, lengths = _ids_and_lengths(ids, attention_mask, self.arch.max_pos)
        task_h = self.task_ids(tasks, int(lengths.size))
        out = torch.empty(int(lengths.size), self.arch.width, dtype=torch.float32, device=self.device)
        lora = C.byref(self.lora) if self.lora is not None else None
        with torch.cuda.device(self.device), _large_call(self.device, int(lengths.sum())):
            for a, b in self._chunks(lengths):
                d_packed, d_cu, cu = self._stage_host(ids_h, lengths, a, b)
                th = torch.from_numpy(np.ascontiguousarray(task_h[a:b]))
                d_task = self._to_device(th)
                ws = self._workspace(self.lib.mq_jina_v3_workspace_bytes(C.byref(self.cfg), d_packed.numel(), b - a))
                L.check(self.lib.mq_encode_jina_v3(C.byref(self.cfg), C.byref(self.w), lora, d_packed.data_ptr(), d_cu.data_ptr(), cu.data_ptr(),
                                                   d_task.data_ptr(), th.data_ptr(), b - a, out[a:b].data_ptr(), 1 if normalize else 0, ws.data_ptr(),
                                                   ws.numel(), self._stream()), "mq_encode_jina_v3")
        return out

    def encode_ids(self, ids: Tensor, attention_mask: Tensor, normalize: bool = True) -> Tensor:
        return self.encode(ids, attention_mask, None, normalize)
