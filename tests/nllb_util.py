"""Shared by tests/test_nllb_host.py and tests/test_nllb_gpu.py: a SentencePiece model of type BPE trained on the spot (a seeded multi-script
corpus, pieces 0-3 = <s> <pad> </s> <unk> like NLLB's), the tokenizer files of a checkpoint directory around it, seeded M2M100 encoders of the
installed `transformers` as the checker, and the fp32 restatement of the tower over the engine's own load-time tensors."""
import json
import math
import os
import random

import torch

LANG = "eng_Latn"

_SCRIPTS = {
    "latin": "abcdefghijklmnopqrstuvwxyz",
    "cyrillic": "абвгдежзийклмнопрстуфхцчшщыэюя",
    "greek": "αβγδεζηθικλμνξοπρστυφχψω",
    "cjk": "日本語中文字漢学生時間東京大人年月火水木金土山川田",
}


def words(rng: random.Random, script: str, n: int):
    abc = _SCRIPTS[script]
    return ["".join(rng.choice(abc) for _ in range(rng.randint(1, 3 if script == "cjk" else 9))) for _ in range(n)]


def corpus(seed: int, n: int, unknown: bool = False):
    """n seeded texts in four scripts: words of a per-script lexicon (so that merges exist), digits and punctuation, irregular spacing;
    unknown = True sprinkles characters the training corpus never saw (they encode as <unk>)"""
    rng = random.Random(seed)
    lex = {s: words(random.Random(1000 + i), s, 60) for i, s in enumerate(_SCRIPTS)}
    out = []
    for _ in range(n):
        s = rng.choice(list(_SCRIPTS))
        toks = []
        for _ in range(rng.randint(1, 12)):
            r = rng.random()
            if r < 0.75:
                toks.append(rng.choice(lex[s]))
            elif r < 0.85:
                toks.append(str(rng.randint(0, 99999)))
            elif r < 0.93:
                toks.append(rng.choice(lex[rng.choice(list(_SCRIPTS))]) + rng.choice(",.!?;:"))
            else:
                toks.append(words(rng, s, 1)[0])
            if unknown and rng.random() < 0.15:    # (one unseen character, or several in a row: SentencePiece joins consecutive <unk> into one)
                toks.append("".join(rng.choice("☃♞€ßñ¿Ωж") for _ in range(rng.choice((1, 1, 2, 3)))) + rng.choice(lex[s]))
        sep = [" " * rng.choice((1, 1, 1, 2, 3)) for _ in toks]
        out.append("".join(t + p for t, p in zip(toks, sep)).rstrip() if rng.random() < 0.8 else "".join(t + p for t, p in zip(toks, sep)))
    return out


def train_bpe(directory: str, vocab_size: int = 400, fairseq_layout: bool = False) -> str:
    """-> directory holding sentencepiece.bpe.model (type BPE) and a tokenizer.json whose added tokens carry the language code, at the id
    transformers' NllbTokenizer gives it: behind the SentencePiece ids shifted by one.  Special pieces: 0-3 = <s> <pad> </s> <unk>, or
    (fairseq_layout, what the published NLLB / XLM-R sentencepiece files carry) <unk> = 0, <s> = 1, </s> = 2 and no <pad>"""
    import sentencepiece as spm
    os.makedirs(directory, exist_ok=True)
    txt = os.path.join(directory, "corpus.txt")
    with open(txt, "w", encoding="utf-8") as f:
        f.write("\n".join(corpus(7, 4000)))
    spm.SentencePieceTrainer.train(input=txt, model_prefix=os.path.join(directory, "sentencepiece.bpe"), model_type="bpe", vocab_size=vocab_size,
                                   character_coverage=1.0, minloglevel=2, num_threads=1,
                                   **(dict(unk_id=0, bos_id=1, eos_id=2, pad_id=-1) if fairseq_layout else dict(bos_id=0, pad_id=1, eos_id=2, unk_id=3)))
    sp = spm.SentencePieceProcessor(model_file=os.path.join(directory, "sentencepiece.bpe.model"))
    assert [sp.id_to_piece(i) for i in range(3)] == (["<unk>", "<s>", "</s>"] if fairseq_layout else ["<s>", "<pad>", "</s>"]) and sp.unk_id() == (0 if fairseq_layout else 3)
    with open(os.path.join(directory, "tokenizer.json"), "w", encoding="utf-8") as f:
        json.dump({"added_tokens": [{"id": len(sp) + 1 + 5, "content": LANG, "special": True}]}, f)
    return directory


def m2m100_encoder(vocab: int, layers: int, mlp_dim: int, seed: int, width: int = 1024, heads: int = 16, bf16_exact: bool = True):
    """the installed transformers' M2M100Encoder with the NLLB-200 encoder's config (pre-LN, ReLU, scaled embeddings, sinusoidal positions) and
    seeded random weights; LayerNorm scales / biases and the biases perturbed so that a mapping mistake shows.  bf16_exact: the GEMM weights and
    the token table are bf16-representable, so that the engine's bf16 copies of them are the same numbers."""
    from transformers import M2M100Config
    from transformers.models.m2m_100.modeling_m2m_100 import M2M100Encoder
    cfg = M2M100Config(vocab_size=vocab, d_model=width, encoder_layers=layers, encoder_ffn_dim=mlp_dim, encoder_attention_heads=heads,
                       decoder_layers=1, activation_function="relu", scale_embedding=True, max_position_embeddings=1024, pad_token_id=1,
                       dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0)
    torch.manual_seed(seed)
    enc = M2M100Encoder(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if name.endswith("embed_tokens.weight"):
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(width))
            elif "layer_norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif p.ndim == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (0.6 / math.sqrt(p.shape[1])))
            if bf16_exact and p.ndim == 2:
                p.copy_(p.to(torch.bfloat16).to(torch.float32))
    return enc


def checkpoint_of(enc, out_dim: int, seed: int, bf16_exact: bool = True):
    """the tower's tensors as open_clip's HFTextEncoder writes them: text.transformer.* (the encoder's own state dict) + text.proj.weight"""
    g = torch.Generator().manual_seed(seed + 2)
    width = enc.config.d_model
    proj = torch.randn(out_dim, width, generator=g) / math.sqrt(width)
    if bf16_exact:
        proj = proj.to(torch.bfloat16).to(torch.float32)
    sd = {"text.transformer." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    sd["text.proj.weight"] = proj
    sd["logit_scale"], sd["logit_bias"] = torch.tensor(2.3), torch.tensor(-10.0)
    return sd, proj


def rows(lengths, vocab: int, ctx: int, seed: int, pad_id: int = 1):
    """right-padded id rows [n, ctx]: language-code id (the largest), random ids, </s> = 2"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), ctx), pad_id, dtype=torch.int64)
    for i, n in enumerate(lengths):
        ids[i, :n] = torch.randint(4, vocab - 1, (n,), generator=g)
        ids[i, 0], ids[i, n - 1] = vocab - 1, 2
    return ids


@torch.no_grad()
def reference_embeddings(enc, proj, ids, pad_id: int = 1, dtype=torch.float32, device="cpu"):
    """open_clip HFTextEncoder.forward: attention_mask = ids != pad, cls_pooler (position 0), linear projection — un-normalised [n, out_dim]"""
    enc = enc.to(device=device, dtype=dtype)
    ids = ids.to(device)
    out = enc(input_ids=ids, attention_mask=(ids != pad_id).long()).last_hidden_state[:, 0]
    return (out @ proj.to(device=device, dtype=dtype).t()).float().cpu()


@torch.no_grad()
def restated_tower(csd, arch, ids, act=torch.relu, pad_id: int = 1):
    """fp32 PyTorch restatement of the engine's dataflow over ITS load-time tensors (towers.nllb_clip_state_dict: CLIP names): per sequence, the
    un-padded rows only; token table + position table; pre-LN blocks with a packed QKV; ln_final on row 0; projection."""
    W, H = arch.width, arch.heads
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (W,), csd[p + ".weight"], csd[p + ".bias"], arch.ln_eps)
    out = []
    for row in ids:
        row = row[row != pad_id]
        T = row.numel()
        x = csd["token_embedding.weight"][row] + csd["positional_embedding"][:T]
        for i in range(arch.layers):
            p = f"transformer.resblocks.{i}."
            q, k, v = (ln(x, p + "ln_1") @ csd[p + "attn.in_proj_weight"].t() + csd[p + "attn.in_proj_bias"]).view(T, 3, H, W // H).unbind(1)
            a = torch.softmax(torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(W // H), dim=-1)
            x = x + torch.einsum("hqk,khd->qhd", a, v).reshape(T, W) @ csd[p + "attn.out_proj.weight"].t() + csd[p + "attn.out_proj.bias"]
            h = act(ln(x, p + "ln_2") @ csd[p + "mlp.c_fc.weight"].t() + csd[p + "mlp.c_fc.bias"])
            x = x + h @ csd[p + "mlp.c_proj.weight"].t() + csd[p + "mlp.c_proj.bias"]
        out.append(ln(x[:1], "ln_final")[0] @ csd["text_projection"])
    return torch.stack(out)


def device_rows(dev, texts, max_length: int):
    """what the tokenisation kernels alone make of `texts` (no host patching): (ids int32 [n, max_length], lengths [n], status [n]) on the host;
    status 1 = the text is left to the host tokeniser.  `dev`: a DeviceSentencePieceTokenizer"""
    m = len(texts)
    with dev._lock, torch.cuda.device(dev.device):
        d_blob, d_off, total = dev._stage(texts)
        d_ids = torch.full((m, max_length), dev.pad_id, dtype=torch.int32, device=dev.device)
        d_meta = torch.empty(2, m, dtype=torch.int32, device=dev.device)
        dev._launch(d_blob, d_off, m, total, max_length, d_ids, d_meta)
        meta = d_meta.cpu().numpy()
        return d_ids.cpu().numpy(), meta[0], meta[1]
