"""Hugging Face (transformers) CLIP naming -> the names the towers load: the encoder layers, the text tower's state dict and the tokenizer files
of the checkpoints that ship under those names (OWL-ViT: engine/owl.py, LanguageBind: engine/languagebind.py)."""
import json
import os
from typing import Dict

import torch

from marqo_amd.engine.archs import ClipTextArch
from marqo_amd.engine.tokenizers import ClipBpeTokenizer
from marqo_amd.engine.tower_weights import _need

Tensor = torch.Tensor


def clip_state_dict(sd: Dict[str, Tensor], prefix: str, layers: int) -> Dict[str, Tensor]:
    """transformers' CLIP-style encoder layers under `prefix` (encoder.layers.N.{self_attn.{q,k,v,out}_proj, layer_norm1, mlp.fc1, mlp.fc2,
    layer_norm2}) -> open_clip's `transformer.resblocks.N.*` names, q | k | v packed, as _clip_blocks loads them"""
    out = {}
    for i in range(layers):
        p, o = f"{prefix}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for kind in ("weight", "bias"):
            out[o + "attn.in_proj_" + kind] = torch.cat([_need(sd, p + f"self_attn.{n}_proj.{kind}").detach().to(torch.float32) for n in "qkv"], dim=0)
            for src, dst in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                             ("mlp.fc2", "mlp.c_proj")):
                out[o + dst + "." + kind] = _need(sd, p + src + "." + kind)
    return out


def clip_text_state_dict(sd: Dict[str, Tensor], prefix: str, projection: str, arch: ClipTextArch) -> Dict[str, Tensor]:
    """the text model under `prefix` (`embeddings.*`, `encoder.layers.N.*`, `final_layer_norm.*`) + sd[projection] -> the open_clip names ClipTextTower loads"""
    out = clip_state_dict(sd, prefix, arch.layers)
    out["token_embedding.weight"] = _need(sd, prefix + "embeddings.token_embedding.weight", (arch.vocab, arch.width))
    out["positional_embedding"] = _need(sd, prefix + "embeddings.position_embedding.weight", (arch.ctx, arch.width))
    out["ln_final.weight"], out["ln_final.bias"] = _need(sd, prefix + "final_layer_norm.weight"), _need(sd, prefix + "final_layer_norm.bias")
    out["text_projection"] = _need(sd, projection, (arch.out_dim, arch.width)).detach().to(torch.float32).t().contiguous()
    return out


def load_tokenizer(directory: str, ctx: int) -> ClipBpeTokenizer:
    """vocab.json + merges.txt of a Hugging Face CLIP tokenizer -> the engine's CLIP BPE tokenizer, after checking that the ids the merges imply
    (byte units, byte units + </w>, merges in order, SOT, EOT) are the ids vocab.json assigns"""
    merges_path, vocab_path = os.path.join(directory, "merges.txt"), os.path.join(directory, "vocab.json")
    for p in (merges_path, vocab_path):
        if not os.path.isfile(p):
            raise FileNotFoundError(f"{p} not found: the OWL-ViT query tokenizer needs vocab.json and merges.txt")
    with open(merges_path, encoding="utf-8") as f:
        lines = f.read().split("\n")
    merges = [tuple(ln.split()) for ln in lines if ln.strip() and not ln.startswith("#version")]
    if any(len(m) != 2 for m in merges):
        raise ValueError(f"{merges_path}: every line must hold two symbols")
    tok = ClipBpeTokenizer(merges, context_length=ctx)
    with open(vocab_path, encoding="utf-8") as f:
        vocab = json.load(f)
    names = {tok.SOT: "<|startoftext|>", tok.EOT: "<|endoftext|>"}
    bad = [(t, i, vocab.get(names.get(t, t))) for t, i in tok.encoder.items() if vocab.get(names.get(t, t)) != i]
    if bad or len(vocab) != len(tok.encoder):
        raise ValueError(f"{vocab_path} does not number the tokens as its merges.txt implies ({len(vocab)} entries against {len(tok.encoder)}; "
                         f"first disagreements (token, implied id, vocab.json id): {bad[:3]})")
    return tok
