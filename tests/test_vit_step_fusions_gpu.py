"""The glue launches of the ViT image step that were folded away, each behind its mq_tune knob:

  pool_strided    the class-token rows of the pooled last block and of the head are read and updated where they lie (row pitch T * W in the skinny
                  GEMMs, a row multiplier in the LayerNorms) instead of through an index vector, two gathers and a scatter
  assemble_stats  the token assembly leaves (mean, rstd) of the rows it stores, so no statistics pass over x runs in front of the first QKV GEMM

Both run the same arithmetic in the same order on the same values, so a knob must not change a single bit of the embeddings.

Geometry: ViT-B/32 (W 768, 12 heads, patch 32, 224 px, T 50) with 2 layers — an ordinary block and the pooled last block — and synthetic weights.
Batches: 1 (one lone image: the skinny-kernel family, LayerNorms in the GEMM prologues), 3 (150 rows: a ragged last row tile, pooled rows in one
skinny tile), 130 (6 500 rows = 40.6 row tiles; above the 128 images from which attention + out-projection run as one launch; pooled rows in row
groups of the skinny kernel).
"""
import dataclasses

import pytest
import torch

from oracle import towers as O
from tests.test_towers_gpu import COS_TIGHT   # the bound tests/test_towers_gpu.py holds this tower to

pytestmark = pytest.mark.gpu

KNOBS = ("pool_strided", "assemble_stats")
BATCHES = (1, 3, 130)


def _cos_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    cos = (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))
    return float((1 - cos).max())


@pytest.fixture(scope="module")
def setup():
    """tower, its 130 images, and the CPU oracle's embeddings of them (computed once; the smaller batches are prefixes)"""
    from marqo_amd.engine import archs, synthetic, towers
    arch, _ = archs.resolve_open_clip("ViT-B-32")
    arch = dataclasses.replace(arch, layers=2)
    sd = synthetic.random_open_clip_state_dict(vision=arch, seed=0)
    g = torch.Generator().manual_seed(31)
    u8 = torch.randint(0, 256, (max(BATCHES), arch.image_size, arch.image_size, 3), generator=g, dtype=torch.uint8)
    cfg = O.VitConfig(arch.image_size, arch.patch_size, arch.width, arch.layers, arch.heads, arch.mlp_dim, arch.out_dim)
    ref = O.vit_forward(sd, cfg, O.preprocess_u8_exact_size(u8))
    tower = towers.VitTower(arch, sd, "cuda")
    assert tower.residual_stream == "bf16"   # the folded LayerNorms (and with them the statistics in question) live on the bf16 stream
    yield tower, u8.cuda(), ref
    for k in KNOBS:
        tower.tune(k, 1)


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("knob", KNOBS)
def test_knob_is_bit_identical(setup, knob, n):
    tower, u8, _ = setup
    try:
        tower.tune(knob, 1)
        on = tower.encode_u8(u8[:n]).cpu()
        tower.tune(knob, 0)
        off = tower.encode_u8(u8[:n]).cpu()
    finally:
        tower.tune(knob, 1)
    assert torch.isfinite(on).all() and on.shape == (n, 512)
    assert torch.equal(on, off), f"{knob}, n={n}: max |diff| = {(on - off).abs().max().item():.3e}"


@pytest.mark.parametrize("n", BATCHES)
def test_all_knobs_off_is_bit_identical(setup, n):
    """... and together (the launch sequence of the parent) against together on"""
    tower, u8, _ = setup
    try:
        on = tower.encode_u8(u8[:n]).cpu()
        for k in KNOBS:
            tower.tune(k, 0)
        off = tower.encode_u8(u8[:n]).cpu()
    finally:
        for k in KNOBS:
            tower.tune(k, 1)
    assert torch.equal(on, off), f"n={n}: max |diff| = {(on - off).abs().max().item():.3e}"


@pytest.mark.parametrize("n", BATCHES)
def test_against_oracle(setup, n):
    tower, u8, ref = setup
    out = tower.encode_u8(u8[:n])
    err = _cos_err(out, ref[:n])
    print(f"n={n}: max(1 - cos) vs oracle = {err:.3e} (bound {COS_TIGHT:.0e})")
    assert err < COS_TIGHT
    assert torch.allclose(out.norm(dim=-1).cpu(), torch.ones(n), atol=1e-5)


@pytest.mark.parametrize("n", (3, 130))
def test_permutation_is_bit_exact(setup, n):
    """permuting the images of a batch permutes the rows of the output, bit for bit (what the request coalescer leans on)"""
    tower, u8, _ = setup
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    assert n < 2 or not torch.equal(perm, torch.arange(n))
    full = tower.encode_u8(u8[:n])
    assert torch.equal(tower.encode_u8(u8[:n][perm.cuda()]), full[perm.cuda()])
