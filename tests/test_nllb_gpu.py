"""NLLB-CLIP on the GPU: the ReLU epilogues of the GEMMs an MQ_ACT_RELU block runs (LayerNorm-folded tiled, skinny, fused-LayerNorm skinny), the
SentencePiece-BPE kernels against the host tokeniser, the text tower at the depth of both models against the installed `transformers` M2M100
encoder, and vectorise() through `model_properties`.

Tower bound (nothing measured on the code under test went into it): (a) = our 1 - cos against the encoder run in fp64, (b) = the same
`transformers` model run by torch in bf16 on the same GPU against it; required (a) <= 2 x (b) — the factor covers the folded LayerNorm and the
bf16 residual stream, which torch's bf16 run does not have.  Random-init towers map every text close to one common direction, so 1 - cos alone
cannot tell a mapping mistake from rounding: the error is also taken against the spread between the texts, rel = max |out - ref| /
min |ref - batch mean|, required <= 2 x torch bf16's and < 0.5 (at 0.5 an embedding would sit as close to the batch mean as to its own reference).
Measured figures per configuration: profiles/r10_nllb_gpu_tests.txt."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import nllb_util as U
from tests.knobs import tuned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTX = 77


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- GEMM epilogues ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,mean", [(500, 4096, 1024, 0.0), (3081, 4096, 1024, 0.3), (333, 8192, 1024, 3.0), (1300, 8192, 1024, -1.0), (97, 4096, 1024, 0.5)])
def test_ln_apply_relu_gemm_equals_layernorm_then_gemm(M, N, K, mean):
    """MQ_EPI_BIAS | MQ_EPI_RELU | MQ_EPI_LN_APPLY (mq_gemm_bf16_ln) with the tolerance rule of its GELU twins, tests/test_ln_fold_gpu.py"""
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(N + K + M)
    x = torch.randn(M, K, device="cuda", generator=g) * 2.0 + mean * 2.0
    x[:, 7] += 40.0
    xb = x.to(torch.bfloat16)
    x = xb.float()
    gam = 1 + 0.2 * torch.randn(K, device="cuda", generator=g)
    bet = 0.1 * torch.randn(K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
    b = 0.1 * torch.randn(N, device="cuda", generator=g)
    eps = 1e-5
    want = torch.relu(torch.nn.functional.layer_norm(x, (K,), gam, bet, eps) @ W.t() + b)
    wf = (W * gam.unsqueeze(0)).to(torch.bfloat16)
    bf, colsum = (b + W @ bet).contiguous(), wf.float().sum(1).contiguous()
    flags = L.MQ_EPI_BIAS | L.MQ_EPI_RELU

    def run():
        out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        stats = torch.empty(M, 2, device="cuda")
        L.check(lib.mq_row_stats(xb.data_ptr(), stats.data_ptr(), M, K, eps, _stream()))
        L.check(lib.mq_gemm_bf16_ln(xb.data_ptr(), K, wf.data_ptr(), K, bf.data_ptr(), colsum.data_ptr(), stats.data_ptr(), out.data_ptr(), N, M, N, K, flags,
                                    _stream()), "mq_gemm_bf16_ln")
        return out
    out = run()
    assert torch.equal(out.view(torch.int16), run().view(torch.int16))
    assert float(out.float().min()) >= 0.0 and float((out == 0).float().mean()) > 0.2          # a ReLU: no negative value, a good share of zeros
    h = torch.nn.functional.layer_norm(x, (K,), gam, bet, eps).to(torch.bfloat16)
    unf = torch.empty_like(out)
    Wb = W.to(torch.bfloat16)
    L.check(lib.mq_gemm_bf16(h.data_ptr(), K, Wb.data_ptr(), K, b.data_ptr(), 0, unf.data_ptr(), N, M, N, K, flags, _stream()))
    scale = want.abs().max().item()
    err_f = (out.float() - want).abs().max().item() / scale
    rms_f = ((out.float() - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()
    rms_u = ((unf.float() - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()
    print(f"M={M} N={N} K={K} mean={mean} relu: folded max {err_f:.2e} rms {rms_f:.2e} | unfolded rms {rms_u:.2e}")
    assert err_f < 2.5e-2 and rms_f < 8e-3
    assert rms_f < 3.0 * rms_u + 1e-3


@pytest.mark.parametrize("M", [1, 3, 17, 32, 50, 80, 200])
def test_skinny_relu_gemms(M):
    """MQ_EPI_BIAS | MQ_EPI_RELU on mq_gemm_small_bf16 (one row group and, M = 200, row groups) and on mq_ln_gemm_small_bf16 (M <= 32), with the
    tolerances of their GELU twins in tests/test_small_m_gpu.py: 2e-2 of the largest value; the fused LayerNorm bit for bit against LayerNorm + GEMM"""
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(500 + M)
    flags = L.MQ_EPI_BIAS | L.MQ_EPI_RELU
    K = 1024
    for N in (4096, 8192):
        A = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        bias = torch.randn(N, device="cuda", generator=g)
        want = torch.relu(A.float() @ W.float().t() + bias)
        out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        L.check(lib.mq_gemm_small_bf16(A.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), 0, out.data_ptr(), N, M, N, K, flags, _stream()), "mq_gemm_small_bf16")
        err = (out.float() - want).abs().max().item() / want.abs().max().item()
        print(f"skinny relu M={M} N={N}: {err:.2e}")
        assert err < 2e-2 and float(out.float().min()) >= 0.0 and float((out == 0).float().mean()) > 0.2
        if M > 32:
            continue
        x = (torch.randn(M, K, device="cuda", generator=g) * 3 + 0.5).to(torch.bfloat16)
        gam = torch.rand(K, device="cuda", generator=g) + 0.5
        bet = torch.randn(K, device="cuda", generator=g) * 0.1
        h = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
        L.check(lib.mq_layernorm_ex(x.data_ptr(), 1, 0, gam.data_ptr(), bet.data_ptr(), h.data_ptr(), 0, M, K, 1e-5, _stream()))
        fused, two = torch.empty_like(out), torch.empty_like(out)
        L.check(lib.mq_ln_gemm_small_bf16(x.data_ptr(), K, 1, gam.data_ptr(), bet.data_ptr(), 1e-5, W.data_ptr(), K, bias.data_ptr(), fused.data_ptr(), N, M, N, K,
                                          flags, 0, _stream()), "mq_ln_gemm_small_bf16")
        L.check(lib.mq_gemm_small_bf16(h.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), 0, two.data_ptr(), N, M, N, K, flags, _stream()))
        assert torch.equal(fused, two)
        ref = torch.relu(torch.nn.functional.layer_norm(x.float(), (K,), gam, bet, 1e-5).to(torch.bfloat16).float() @ W.float().t() + bias)
        assert (fused.float() - ref).abs().max().item() / ref.abs().max().item() < 3e-2


# ---- device SentencePiece-BPE --------------------------------------------------------------------------------------------------------
# two special-piece layouts: the issue's (pieces 0-3 = <s> <pad> </s> <unk>) and the published NLLB / XLM-R files' (<unk> = 0, <s> = 1, </s> = 2)
@pytest.fixture(scope="module", params=["issue", "fairseq"])
def bpe_dir(request, tmp_path_factory):
    return U.train_bpe(str(tmp_path_factory.mktemp("nllb_bpe_" + request.param)), fairseq_layout=request.param == "fairseq")


def test_device_bpe_equals_host_tokenizer(bpe_dir):
    from marqo_amd.engine.gpu_tokenizers import DeviceSentencePieceTokenizer
    from marqo_amd.engine.tokenizers import NllbTokenizer
    from marqo_amd.s2_inference.open_clip_model import HfClipTokenizer
    host = NllbTokenizer(bpe_dir)
    dev = DeviceSentencePieceTokenizer(host, DEV)
    assert dev.kind == "nllb"
    # (1) a corpus of characters the device route claims only (four scripts, digits, punctuation, characters the vocabulary never saw): nothing may be
    # left to the host, and the kernels' own rows — not the patched ones — are compared
    texts = U.corpus(31, 3000, unknown=True)
    want = HfClipTokenizer(host, CTX).ids(texts)
    ids, lens, status = U.device_rows(dev, texts, CTX)
    assert int(status.sum()) == 0
    np.testing.assert_array_equal(ids, want)
    np.testing.assert_array_equal(lens, (want != 1).sum(axis=1))
    # (2) what the kernels must hand back or frame right: flagged code points (a combining mark that composes; a conjoining jamo; U+2581 itself), a
    # word beyond the per-word scratch, the empty and the whitespace-only text, more than 77 pieces
    odd = ["e\u0301cole", "\u1161", "a\u2581b", "z" * 300, "", "  \t ", " ".join(U.corpus(32, 40)), "ok then", "ab ☃♞ cd € ß"]
    ids, lens, status = U.device_rows(dev, odd, CTX)
    np.testing.assert_array_equal(status, [1, 1, 1, 1, 0, 0, 0, 0, 0])
    want = HfClipTokenizer(host, CTX).ids(odd)
    np.testing.assert_array_equal(ids[4:], want[4:])
    np.testing.assert_array_equal(lens[4:], [2, 2, CTX, int((want[7] != 1).sum()), int((want[8] != 1).sum())])
    unk = host.sp.unk_id() + 1 if host.sp.unk_id() else 3
    assert int((ids[8] == unk).sum()) == 3                                   # unseen characters in a row are ONE <unk>, apart ones are not
    d_ids, d_lens = dev.encode_device(odd, CTX)            # the public route: flagged texts patched in from the host tokeniser
    np.testing.assert_array_equal(d_ids.cpu().numpy(), want)
    np.testing.assert_array_equal(d_lens.numpy(), (want != 1).sum(axis=1))
    np.testing.assert_array_equal(dev(odd, CTX)["input_ids"], want[:, :int((want != 1).sum(axis=1).max())])


# ---- the tower -----------------------------------------------------------------------------------------------------------------------
VOCAB = 3000
LENGTHS = [3, 4, 5, 7, 9, 12, 16, 20, 25, 31, 33, 40, 48, 56, 64, 70, 76, 77, 6, 11, 77, 50, 3, 29]


def _cos_err(a, b):
    a, b = a.double(), b.double()
    return 1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def _rel(out, ref):
    return float((out.double() - ref.double()).norm(dim=-1).max() / (ref.double() - ref.double().mean(0, keepdim=True)).norm(dim=-1).min())


def tower_case(hf_name: str, report=None):
    """one configuration, both residual-stream forms, batch + single-sequence calls -> the measured figures; asserts the bound of the module docstring"""
    from marqo_amd.engine import towers
    arch = replace(archs.NLLB_TEXT_ARCHS[hf_name], vocab=VOCAB)
    enc = U.m2m100_encoder(VOCAB, arch.layers, arch.mlp_dim, seed=arch.layers)
    sd, proj = U.checkpoint_of(enc, arch.out_dim, seed=arch.layers)
    ids = U.rows(LENGTHS, VOCAB, CTX, seed=9)
    ref = U.reference_embeddings(enc, proj, ids, dtype=torch.float64, device=DEV)
    tbf = U.reference_embeddings(enc, proj, ids, dtype=torch.bfloat16, device=DEV)
    b_cos, b_rel = float(_cos_err(tbf, ref).max()), _rel(tbf, ref)
    tw = towers.NllbTextTower(arch, sd, DEV)
    figures = {"config": f"{arch.layers} x {arch.mlp_dim}", "torch_bf16": (b_cos, b_rel), "policy": (tw.residual_stream, tw.residual_stream_error)}
    for stream in (2, 1):
        tw.cfg.enc.residual_stream = stream
        tw._graphs.clear()
        out = tw.encode_ids(ids, normalize=False).cpu()
        a_cos, a_rel = float(_cos_err(out, ref).max()), _rel(out, ref)
        one = torch.cat([tw.encode_ids(ids[i:i + 1], normalize=False).cpu() for i in (0, 7, 17)])       # single-sequence calls: the skinny GEMMs, a captured graph
        o_cos, o_rel = float(_cos_err(one, ref[[0, 7, 17]]).max()), float((one.double() - ref[[0, 7, 17]].double()).norm(dim=-1).max() /
                                                                         (ref.double() - ref.double().mean(0, keepdim=True)).norm(dim=-1).min())
        name = "bf16 stream" if stream == 1 else "fp32 stream"
        figures[name] = (a_cos, a_rel, o_cos, o_rel)
        line = (f"{hf_name} ({arch.layers} x {arch.mlp_dim}) {name}: (a) ours max(1-cos) {a_cos:.3e} rel {a_rel:.3e} | single-sequence {o_cos:.3e} rel {o_rel:.3e} | "
                f"(b) torch bf16 max(1-cos) {b_cos:.3e} rel {b_rel:.3e}")
        print(line)
        if report is not None:
            report.append(line)
        assert a_cos <= 2 * b_cos and o_cos <= 2 * b_cos, line
        assert a_rel <= 2 * b_rel and o_rel <= 2 * b_rel and a_rel < 0.5 and o_rel < 0.5, line
        normed = tw.encode_ids(ids)
        torch.testing.assert_close(normed.cpu(), torch.nn.functional.normalize(out, dim=-1), rtol=1e-5, atol=1e-6)
        d = tw.encode_device(ids.to(DEV, torch.int32), (ids != 1).sum(1), normalize=False).cpu()          # ids packed on the device: the same rows
        assert torch.equal(d, out)
    return figures


@pytest.mark.parametrize("hf_name", ["facebook/nllb-200-distilled-600M", "facebook/nllb-200-distilled-1.3B"])
def test_tower_against_m2m100_encoder(hf_name):
    tower_case(hf_name)


def test_fp8_tower_is_refused():
    from marqo_amd.engine import synthetic, towers
    arch = replace(archs.NLLB_TEXT_ARCHS["facebook/nllb-200-distilled-600M"], vocab=64, layers=1)
    with pytest.raises(ValueError, match="bf16 operands only"):
        towers.NllbTextTower(arch, synthetic.random_open_clip_state_dict(vision=None, text=arch, seed=0), DEV, precision="fp8")


# ---- vectorise() -----------------------------------------------------------------------------------------------------------------------
def test_vectorise_through_model_properties(bpe_dir, tmp_path, monkeypatch):
    """synthetic weights + the trained BPE model in the repo's directory under the model dir: texts (device and host tokenisation), images"""
    import shutil
    from PIL import Image
    from marqo_amd.s2_inference import s2_inference as s2i
    d = tmp_path / "hf-hub" / "visheratin" / "nllb-clip-base-siglip"
    d.mkdir(parents=True)
    for f in ("sentencepiece.bpe.model", "tokenizer.json"):
        shutil.copy(os.path.join(bpe_dir, f), d / f)
    monkeypatch.setenv("MARQO_AMD_MODEL_DIR", str(tmp_path))
    monkeypatch.setenv("MARQO_AMD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"name": "hf-hub:visheratin/nllb-clip-base-siglip", "type": "open_clip", "dimensions": 768}
    texts = U.corpus(41, 24) + ["école de paris", "one"]
    try:
        s2i.clear_loaded_models()
        dev = np.asarray(s2i.vectorise("nllb-clip-test", texts, model_properties=props, device=DEV))
        model = next(iter(s2i._available_models.values()))[s2i.AvailableModelsKey.model]
        kind = getattr(getattr(model, "_device_tokenizer", None), "kind", None)
        one = np.asarray(s2i.vectorise("nllb-clip-test", texts[3], model_properties=props, device=DEV))
        rng = np.random.default_rng(0)
        pil = [Image.fromarray(rng.integers(0, 255, (300, 400, 3), dtype=np.uint8)) for _ in range(2)]
        img = np.asarray(s2i.vectorise("nllb-clip-test", pil, model_properties=props, device=DEV, modality=s2i.Modality.IMAGE))
        s2i.clear_loaded_models()
        monkeypatch.setenv("MARQO_AMD_HOST_TOKENIZER", "1")
        host = np.asarray(s2i.vectorise("nllb-clip-test", texts, model_properties=props, device=DEV))
        with pytest.raises(Exception, match="bf16 operands only"):
            s2i.vectorise("nllb-clip-fp8", texts, model_properties=dict(props, enginePrecision="fp8"), device=DEV)
    finally:
        s2i.clear_loaded_models()
    assert dev.shape == (len(texts), 768) and img.shape == (2, 768) and one.shape == (1, 768)
    np.testing.assert_allclose(np.linalg.norm(dev, axis=-1), 1.0, atol=1e-5)
    np.testing.assert_allclose(np.linalg.norm(img, axis=-1), 1.0, atol=1e-5)
    np.testing.assert_array_equal(dev, host)                       # identical ids on both routes -> identical embeddings
    assert float(1 - (one[0] * dev[3]).sum()) < 1e-4               # the single-query route (host tokenisation, skinny GEMMs, captured graph)
    assert float(np.abs(dev - dev.mean(0)).max()) > 1e-3           # the texts do differ
    assert kind == "nllb"                                          # (the first load did tokenise on the device)


# ---- MQ_ACT_RELU through mq_encoder_forward itself ----------------------------------------------------------------------------------
def test_relu_encoder_with_the_panel_gemm_knob_on():
    """a 768-wide MQ_ACT_RELU encoder over fixed-length sequences that fill the chip, with the (opt-in) one-workgroup-per-sequence GEMMs asked for: the
    panel kernel has no ReLU epilogue, so fc1 keeps the tiled GEMM — a result, the same bits as with the knob off"""
    import ctypes as C
    from marqo_amd.engine import synthetic, towers
    lib = L.load()
    W, F, H, nseq, T = 768, 3072, 12, 256, 16
    sd = {}
    synthetic._resblocks(sd, "t.", 2, W, F, torch.Generator().manual_seed(3))
    holder = towers._Holder(torch.device(DEV))
    blocks = towers._clip_blocks(holder, sd, "t.", 2, W, F, H)
    cfg = towers._encoder_cfg(W, 2, H, F, False, False, L.MQ_MASK_NONE, 1e-5)
    cfg.act, cfg.residual_stream = L.MQ_ACT_RELU, 1
    x0 = torch.randn(nseq * T, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)).to(torch.bfloat16)
    ws = torch.empty(lib.mq_encoder_workspace_bytes(C.byref(cfg), nseq * T, nseq) + 256, dtype=torch.uint8, device=DEV)
    outs = []
    for knob in (0, 1):
        with tuned(panel_gemm=knob):
            x = x0.clone()
            L.check(lib.mq_encoder_forward(C.byref(cfg), blocks, x.data_ptr(), nseq * T, None, nseq, T, T, ws.data_ptr(), ws.numel(), _stream()), "mq_encoder_forward")
            torch.cuda.synchronize()
            outs.append(x)
    assert torch.isfinite(outs[1].float()).all() and not torch.equal(outs[1], x0)
    assert torch.equal(outs[0], outs[1])
