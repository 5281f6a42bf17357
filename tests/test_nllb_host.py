"""NLLB-CLIP without a GPU: the host tokeniser against the `sentencepiece` wheel (and `transformers`' NllbTokenizer where it can be built), the
SentencePiece-BPE functions the device kernels instantiate (compiled for the host) against the same wheel, architecture resolution, the
load-time transforms of the text tower against the installed `transformers` M2M100 encoder, and the argument checks of MQ_ACT_RELU."""
import ctypes as C
import json
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from marqo_amd.engine.tokenizers import NllbTokenizer, _clean_text
from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
from marqo_amd.s2_inference.open_clip_model import OPEN_CLIP, HfClipTokenizer
from tests import nllb_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX = 77


# two special-piece layouts: the issue's (pieces 0-3 = <s> <pad> </s> <unk>) and the one the published NLLB / XLM-R sentencepiece files carry
# (<unk> = 0, <s> = 1, </s> = 2: SentencePiece id 0 becomes the fairseq <unk> = 3, every other id is shifted by one)
@pytest.fixture(scope="module", params=["issue", "fairseq"])
def bpe_dir(request, tmp_path_factory):
    return U.train_bpe(str(tmp_path_factory.mktemp("nllb_bpe_" + request.param)), fairseq_layout=request.param == "fairseq")


def _expected_rows(tok, texts, ctx):
    out = np.full((len(texts), ctx), 1, dtype=np.int64)
    for i, t in enumerate(texts):
        ids = [tok.lang_id] + [p + 1 if p else 3 for p in tok.sp.encode(t)][: ctx - 2] + [2]
        out[i, :len(ids)] = ids
    return out


# ---- host tokeniser ------------------------------------------------------------------------------------------------------------
def test_host_tokenizer_equals_sentencepiece_wheel(bpe_dir):
    tok = NllbTokenizer(bpe_dir)
    assert tok.lang_id == len(tok.sp) + 1 + 5          # read from tokenizer.json by its string
    texts = U.corpus(11, 300, unknown=True) + ["", "   ", "a", " ".join(U.corpus(12, 40))]          # (the last one: far more than 77 pieces)
    rows = HfClipTokenizer(tok, CTX)(texts)
    assert rows.shape == (len(texts), CTX) and rows.dtype == np.int64
    np.testing.assert_array_equal(rows, _expected_rows(tok, texts, CTX))
    assert (rows[:, 0] == tok.lang_id).all() and rows[-1, CTX - 1] == 2 and (rows[-1] != 1).all()   # truncation keeps the language code and </s>
    np.testing.assert_array_equal(rows[-4, :3], [tok.lang_id, 2, 1])                                  # empty text: language code, </s>, padding
    unk = tok.sp.unk_id() + 1 if tok.sp.unk_id() else 3                                                # <unk>: SentencePiece id 3 + 1, or 0 -> fairseq's 3
    assert unk in rows
    two = HfClipTokenizer(tok, CTX)(["ab ☃♞ cd"])[0]                                                    # unseen characters in a row are ONE <unk> (the wheel joins them), apart ones are not
    assert int((two == unk).sum()) == 1 and int((HfClipTokenizer(tok, CTX)(["ab ☃ ♞ cd"])[0] == unk).sum()) == 2


def test_host_tokenizer_needs_the_language_code(bpe_dir, tmp_path):
    shutil.copy(os.path.join(bpe_dir, "sentencepiece.bpe.model"), tmp_path / "sentencepiece.bpe.model")
    with pytest.raises(FileNotFoundError, match="eng_Latn"):
        NllbTokenizer(str(tmp_path))


def test_host_tokenizer_equals_transformers(bpe_dir):
    """the installed transformers' NllbTokenizer, built on tokenizers.models.BPE from the same vocabulary: the pieces at SentencePiece id + 1 behind the
    four fairseq specials, the merges and the normaliser's character map as transformers itself extracts them from the sentencepiece file.  Texts as
    open_clip's clean_fn hands them over (whitespace cleaned), rows with max_length = 77, padding = 'max_length', truncation = True."""
    transformers = pytest.importorskip("transformers")
    try:
        from transformers.convert_slow_tokenizer import SentencePieceExtractor
        ex = SentencePieceExtractor(os.path.join(bpe_dir, "sentencepiece.bpe.model")).extract(None)
        merges, charsmap = ex["merges"], ex["_spm_precompiled_charsmap"]
    except (ImportError, AttributeError, KeyError, TypeError) as e:
        pytest.skip(f"transformers {transformers.__version__} has no SentencePieceExtractor(...).extract(None) -> merges / _spm_precompiled_charsmap: {e!r}")
    tok = NllbTokenizer(bpe_dir)
    vocab = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}
    for i in range(len(tok.sp)):
        vocab.setdefault(tok.sp.id_to_piece(i), i + 1)
    hf = transformers.NllbTokenizer(vocab=vocab, merges=merges, _spm_precompiled_charsmap=charsmap)
    lang = hf.convert_tokens_to_ids(U.LANG)
    assert isinstance(lang, int) and lang > len(tok.sp)
    tok.lang_id = lang              # (this vocabulary's own id of the language code, as tokenizer.json's added tokens would state it)
    # unknown characters (adjacent ones included) where <unk> is SentencePiece id 0, as in the published files: both sides write fairseq's 3.  Under
    # the other layout the issue defines <unk> as SentencePiece id 3 + 1 = 4, which a vocabulary with one <unk> entry cannot say: known characters only
    fairseq = tok.sp.unk_id() == 0
    texts = [_clean_text(t) for t in U.corpus(13, 1000, unknown=fairseq) + [" ".join(U.corpus(12, 40)), "a"]]
    want = np.asarray(hf(texts, max_length=CTX, padding="max_length", truncation=True)["input_ids"])
    assert want.shape == (len(texts), CTX) and (want[:, 0] == lang).all() and (not fairseq or 3 in want)
    np.testing.assert_array_equal(HfClipTokenizer(tok, CTX).ids(texts), want)


# ---- the device algorithm, compiled for the host ------------------------------------------------------------------------------------
class _HostVocab(C.Structure):
    _fields_ = L.SentencePieceVocab._fields_


def test_device_bpe_algorithm_on_the_host_equals_sentencepiece(bpe_dir, tmp_path):
    from marqo_amd.engine.gpu_tokenizers import build_sentencepiece_table
    so = tmp_path / "libspbpe.so"
    subprocess.run(["g++", "-O2", "-fPIC", "-std=c++17", "-Wall", "-shared", "-o", str(so), os.path.join(ROOT, "marqo_amd", "csrc", "tokenize_bpe_host.cpp")],
                   check=True)
    lib = C.CDLL(str(so))
    lib.mq_host_sentencepiece_bpe.restype = C.c_int
    lib.mq_host_sentencepiece_bpe.argtypes = [C.POINTER(_HostVocab), C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    tok = NllbTokenizer(bpe_dir)
    t = build_sentencepiece_table(tok.sp, bpe=True)
    keep = [np.ascontiguousarray(t[k]) for k in ("slots", "pool", "scores", "nmap", "npool", "ccc")]
    p = [a.ctypes.data for a in keep]
    v = _HostVocab(d_slots=p[0], d_pool=p[1], d_score=p[2], d_nmap=p[3], d_npool=p[4], d_ccc=p[5], n_slots=t["n_slots"], unk_id=t["unk_id"],
                   unk_score=t["unk_score"], add_dummy_prefix=t["add_dummy_prefix"], remove_extra_ws=t["remove_extra_ws"],
                   max_piece_bytes=t["max_piece_bytes"], prefix_id=tok.lang_id, suffix_id=2, pad_id=1, id_offset=1, unk_out=t["unk_id"] + 1 if t["unk_id"] else 3)
    texts = U.corpus(21, 2000, unknown=True) + ["", " ", "x" * 40, " ".join(U.corpus(22, 40)), "ab ☃♞ cd", "€€€"]
    want = _expected_rows(tok, texts, CTX)
    row = np.zeros(CTX, dtype=np.int32)
    st = C.c_int32(0)
    bad = 0
    for i, text in enumerate(texts):
        b = text.encode("utf-8")
        n = lib.mq_host_sentencepiece_bpe(C.byref(v), b, len(b), CTX, row.ctypes.data, CTX, C.byref(st))
        assert st.value == 0, text
        assert n == int((want[i] != 1).sum())
        bad += int(not np.array_equal(row, want[i]))
    assert bad == 0
    # a word beyond the per-word scratch and a flagged code point (a combining mark that composes with its neighbour) go to the host tokeniser
    for text in ("y" * 200, "e\u0301"):
        b = text.encode("utf-8")
        lib.mq_host_sentencepiece_bpe(C.byref(v), b, len(b), CTX, row.ctypes.data, CTX, C.byref(st))
        assert st.value == 1, text


def test_bpe_table_refuses_what_the_device_cannot_merge_per_word(bpe_dir, tmp_path):
    import sentencepiece as spm
    from marqo_amd.engine.gpu_tokenizers import build_sentencepiece_table
    tok = NllbTokenizer(bpe_dir)
    with pytest.raises(ValueError, match="type"):
        build_sentencepiece_table(tok.sp, bpe=False)                      # a BPE model is no unigram model
    txt = tmp_path / "c.txt"
    txt.write_text("\n".join(["new york is new york", "san jose or new york", "in san jose"] * 200), encoding="utf-8")
    spm.SentencePieceTrainer.train(input=str(txt), model_prefix=str(tmp_path / "ws"), model_type="bpe", vocab_size=45, split_by_whitespace=False,
                                   character_coverage=1.0, minloglevel=2, num_threads=1)
    sp = spm.SentencePieceProcessor(model_file=str(tmp_path / "ws.model"))
    assert any("▁" in sp.id_to_piece(i)[1:] for i in range(len(sp)))
    with pytest.raises(ValueError, match="U\\+2581"):
        build_sentencepiece_table(sp, bpe=True)                           # pieces that span words: the whole vocabulary stays on the host


# ---- architecture resolution --------------------------------------------------------------------------------------------------------
def _config(tmp_path, timm, hf_name, embed_dim, **text):
    cfg = {"model_cfg": {"embed_dim": embed_dim, "init_logit_bias": -10, "custom_text": True,
                         "vision_cfg": {"image_size": 384, "timm_model_name": timm, "timm_model_pretrained": False, "timm_pool": "map", "timm_proj": "none"},
                         "text_cfg": {"hf_model_name": hf_name, "hf_tokenizer_name": hf_name, "hf_proj_type": "linear", "hf_pooler_type": "cls_pooler", **text}},
           "preprocess_cfg": {"mean": [0.5, 0.5, 0.5], "std": [0.5, 0.5, 0.5]}}
    (tmp_path / "open_clip_config.json").write_text(json.dumps(cfg))
    return str(tmp_path)


def _model(name="hf-hub:visheratin/nllb-clip-base-siglip", dims=768):
    return OPEN_CLIP(device="cpu", model_properties={"name": name, "type": "open_clip", "dimensions": dims})


@pytest.mark.parametrize("timm, hf, dim, layers, mlp, width", [
    ("vit_base_patch16_siglip_384", "facebook/nllb-200-distilled-600M", 768, 12, 4096, 768),
    ("vit_so400m_patch14_siglip_384", "facebook/nllb-200-distilled-1.3B", 1152, 24, 8192, 1152)])
def test_resolve_archs_from_open_clip_config(tmp_path, timm, hf, dim, layers, mlp, width):
    v, t = _model()._resolve_archs("hf-hub:visheratin/nllb-clip-base-siglip", None, _config(tmp_path, timm, hf, dim))
    assert isinstance(v, archs.VitArch) and (v.image_size, v.width, v.pool, v.out_dim) == (384, width, "map", dim)
    assert isinstance(t, archs.NllbTextArch)
    assert (t.vocab, t.ctx, t.width, t.layers, t.heads, t.mlp_dim, t.out_dim, t.pad_id, t.ln_eps) == (256206, 77, 1024, layers, 16, mlp, dim, 1, 1e-5)


@pytest.mark.parametrize("name, layers, dim", [("hf-hub:visheratin/nllb-clip-base-siglip", 12, 768), ("hf-hub:visheratin/nllb-siglip-mrl-base", 12, 768),
                                               ("hf-hub:visheratin/nllb-clip-large-siglip", 24, 1152), ("hf-hub:visheratin/nllb-siglip-mrl-large", 24, 1152)])
def test_resolve_archs_table_fallback(name, layers, dim):
    v, t = _model(name, dim)._resolve_archs(name, None, None)
    assert isinstance(t, archs.NllbTextArch) and (t.layers, t.out_dim, v.out_dim, v.image_size, v.pool) == (layers, dim, dim, 384, "map")


def test_resolve_archs_refusals_stay(tmp_path):
    m = _model()
    name = "hf-hub:visheratin/nllb-clip-base-siglip"
    a, b, c, d = (tmp_path / x for x in "abcd")
    for x in (a, b, c, d):
        x.mkdir()
    with pytest.raises(InvalidModelPropertiesError, match="only plain CLIP ViT"):     # another Hugging Face text tower behind a SigLIP trunk
        m._resolve_archs(name, None, _config(a, "vit_base_patch16_siglip_384", "xlm-roberta-base", 768))
    with pytest.raises(InvalidModelPropertiesError, match="cls_pooler"):
        m._resolve_archs(name, None, _config(b, "vit_base_patch16_siglip_384", "facebook/nllb-200-distilled-600M", 768, hf_pooler_type="mean_pooler"))
    with pytest.raises(InvalidModelPropertiesError, match="linear"):
        m._resolve_archs(name, None, _config(c, "vit_base_patch16_siglip_384", "facebook/nllb-200-distilled-600M", 768, hf_proj_type="mlp"))
    cfg = json.loads(open(os.path.join(_config(d, "x", "xlm-roberta-base", 512), "open_clip_config.json")).read())     # plain ViT + xlm-roberta-base
    cfg["model_cfg"]["vision_cfg"] = {"image_size": 224, "layers": 12, "width": 768, "patch_size": 32}
    (d / "open_clip_config.json").write_text(json.dumps(cfg))
    with pytest.raises(InvalidModelPropertiesError, match="only plain CLIP ViT"):
        m._resolve_archs(name, None, str(d))


def test_preprocess_cfg_on_disk_decides(tmp_path):
    a, b, c = (tmp_path / x for x in "abc")
    for x in (a, b, c):
        x.mkdir()
    assert OPEN_CLIP._preprocess_cfg_on_disk(str(tmp_path)) is None and OPEN_CLIP._preprocess_cfg_on_disk(None) is None     # no file: the caller's choice
    d = _config(a, "vit_base_patch16_siglip_384", "facebook/nllb-200-distilled-600M", 768)
    assert OPEN_CLIP._preprocess_cfg_on_disk(d) == ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), "shortest", "bicubic")                 # named fields + open_clip's defaults
    cfg = json.loads((a / "open_clip_config.json").read_text())
    cfg["preprocess_cfg"] = {"mean": [0.4, 0.5, 0.6], "std": [0.2, 0.3, 0.4], "interpolation": "bilinear", "resize_mode": "squash"}
    (b / "open_clip_config.json").write_text(json.dumps(cfg))
    assert OPEN_CLIP._preprocess_cfg_on_disk(str(b)) == ((0.4, 0.5, 0.6), (0.2, 0.3, 0.4), "squash", "bilinear")
    del cfg["preprocess_cfg"]
    (c / "open_clip_config.json").write_text(json.dumps(cfg))
    assert OPEN_CLIP._preprocess_cfg_on_disk(str(c)) == (archs.OPENAI_DATASET_MEAN, archs.OPENAI_DATASET_STD, "shortest", "bicubic")
    cfg["preprocess_cfg"] = {"interpolation": "lanczos"}
    (c / "open_clip_config.json").write_text(json.dumps(cfg))
    with pytest.raises(InvalidModelPropertiesError, match="preprocess_cfg"):
        OPEN_CLIP._preprocess_cfg_on_disk(str(c))


def test_fp8_is_refused_at_load():
    m = OPEN_CLIP(device="cuda", model_properties={"name": "hf-hub:visheratin/nllb-clip-base-siglip", "type": "open_clip", "dimensions": 768,
                                                   "enginePrecision": "fp8"})
    with pytest.raises(InvalidModelPropertiesError, match="bf16 operands only"):
        m._load_necessary_components()


# ---- load-time transforms, pinned to the installed transformers M2M100 encoder ----------------------------------------------------
def test_load_time_transforms_equal_m2m100_encoder():
    from transformers.models.m2m_100.modeling_m2m_100 import M2M100SinusoidalPositionalEmbedding
    from marqo_amd.engine.towers import nllb_clip_state_dict
    arch = replace(archs.NLLB_TEXT_ARCHS["facebook/nllb-200-distilled-600M"], vocab=300, width=128, heads=2, layers=3, mlp_dim=256, out_dim=64)
    enc = U.m2m100_encoder(arch.vocab, arch.layers, arch.mlp_dim, seed=5, width=arch.width, heads=arch.heads, bf16_exact=False)
    sd, proj = U.checkpoint_of(enc, arch.out_dim, seed=5, bf16_exact=False)
    csd = nllb_clip_state_dict(arch, sd)
    # scaled token table, sinusoidal positions from padding_idx + 1 on, packed qkv
    emb = sd["text.transformer.embed_tokens.weight"]
    torch.testing.assert_close(csd["token_embedding.weight"], emb * (arch.width ** 0.5), rtol=0, atol=0)
    pe = M2M100SinusoidalPositionalEmbedding(1024, arch.width, 1)
    ids = torch.full((1, arch.ctx), 7)
    torch.testing.assert_close(csd["positional_embedding"], pe(input_ids=ids)[0].float(), rtol=0, atol=0)
    assert pe.offset == arch.pos_offset and csd["positional_embedding"].shape == (arch.ctx, arch.width)
    big = archs.NLLB_TEXT_ARCHS["facebook/nllb-200-distilled-1.3B"]
    torch.testing.assert_close(big.position_table(), M2M100SinusoidalPositionalEmbedding(1024, 1024, 1)(input_ids=ids)[0].float(), rtol=0, atol=0)
    p = "text.transformer.layers.1.self_attn."
    torch.testing.assert_close(csd["transformer.resblocks.1.attn.in_proj_weight"],
                               torch.cat([sd[p + "q_proj.weight"], sd[p + "k_proj.weight"], sd[p + "v_proj.weight"]]), rtol=0, atol=0)
    torch.testing.assert_close(csd["transformer.resblocks.1.attn.in_proj_bias"][arch.width:2 * arch.width], sd[p + "k_proj.bias"], rtol=0, atol=0)
    # the engine's dataflow over those tensors (un-padded rows, row 0 pooled) equals the padded, masked encoder + cls pooler + projection
    rows = U.rows([3, 9, 40, 77, 2], arch.vocab, arch.ctx, seed=3)
    ref = U.reference_embeddings(enc, proj, rows)
    got = U.restated_tower(csd, arch, rows)
    assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    cos = torch.nn.functional.cosine_similarity(got.double(), ref.double(), dim=-1)
    assert float((1 - cos).max()) < 1e-9
    # ... and the restatement notices what the GPU test's sabotages break: GELU in place of ReLU, an unscaled table, dropped positions
    for broken in (U.restated_tower(csd, arch, rows, act=torch.nn.functional.gelu),
                   U.restated_tower({**csd, "token_embedding.weight": emb}, arch, rows),
                   U.restated_tower({**csd, "positional_embedding": torch.zeros_like(csd["positional_embedding"])}, arch, rows)):
        assert float((1 - torch.nn.functional.cosine_similarity(broken.double(), ref.double(), dim=-1)).max()) > 1e-4


def test_synthetic_state_dict_has_the_checkpoint_keys():
    from marqo_amd.engine import synthetic
    from marqo_amd.engine.towers import nllb_clip_state_dict
    for base in archs.NLLB_TEXT_ARCHS.values():
        arch = replace(base, vocab=64, layers=2)
        sd = synthetic.random_open_clip_state_dict(vision=None, text=arch, seed=0)
        assert "text.proj.weight" in sd and "text.transformer.layers.1.final_layer_norm.bias" in sd and "logit_bias" in sd
        assert sd["text.transformer.layers.0.fc1.weight"].shape == (arch.mlp_dim, 1024) and sd["text.proj.weight"].shape == (arch.out_dim, 1024)
        csd = nllb_clip_state_dict(arch, sd)
        assert csd["text_projection"].shape == (1024, arch.out_dim) and csd["transformer.resblocks.1.mlp.c_proj.weight"].shape == (1024, arch.mlp_dim)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_encoder_argument_checks_for_relu():
    lib = L.load()
    assert L.MQ_ACT_RELU == 4 and lib.mq_abi_version() == 15
    ok = L.EncoderCfg(width=1024, layers=12, heads=16, mlp_dim=4096, act=L.MQ_ACT_RELU, post_ln=0, mask=0, ln_eps=1e-5, precision=L.MQ_PREC_BF16)
    assert lib.mq_encoder_forward(C.byref(ok), None, None, 0, None, 0, 0, 0, None, 0, None) == -1
    assert b"null pointer" in lib.mq_last_error()                    # the configuration itself passed: the next check speaks
    assert lib.mq_encoder_workspace_bytes(C.byref(ok), 100, 2) > 0
    scale = (C.c_float * 24)()
    f8 = L.EncoderCfg(width=1024, layers=12, heads=16, mlp_dim=4096, act=L.MQ_ACT_RELU, post_ln=0, mask=0, ln_eps=1e-5, precision=L.MQ_PREC_FP8,
                      d_fp8_act_scale=C.cast(scale, C.c_void_p))
    assert lib.mq_encoder_forward(C.byref(f8), None, None, 0, None, 0, 0, 0, None, 0, None) == -1
    assert b"MQ_ACT_RELU" in lib.mq_last_error()
    for bad in (dict(post_ln=1), dict(mlp_glu=1)):
        cfg = L.EncoderCfg(**{**dict(width=1024, layers=12, heads=16, mlp_dim=4096, act=L.MQ_ACT_RELU, post_ln=0, mask=0, ln_eps=1e-5), **bad})
        assert lib.mq_encoder_forward(C.byref(cfg), None, None, 0, None, 0, 0, 0, None, 0, None) == -1 and b"MQ_ACT_RELU" in lib.mq_last_error()
    assert hasattr(lib, "mq_tokenize_sentencepiece_bpe")
    v = L.SentencePieceVocab()
    assert lib.mq_tokenize_sentencepiece_bpe(C.byref(v), None, None, 1, 0, 77, None, 77, None, None, None, 0, None) == -1
    assert b"bad vocabulary tables" in lib.mq_last_error()
