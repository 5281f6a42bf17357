"""ConvNeXt CLIP image towers: images/s of the HIP tower (one mq_encode_convnext_u8 call per batch) against the same tower written in torch bf16,
channels_last (F.conv2d / F.linear: MIOpen / hipBLASLt — how open_clip runs it), both in this process, from resident uint8 images, timed with
device events after warm-up.  The torch tower is a yardstick only; it is never on the product path.

  python tools/convnext_bench.py [--archs convnext_base_w,convnext_large_d_320,convnext_xxlarge] [--batches 64,128] [--iters 10] [--no-torch]

Prints one JSON line per (arch, batch)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marqo_amd.engine import archs, synthetic, towers  # noqa: E402
from marqo_amd.engine.archs import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
DEV = "cuda:0"


class TorchConvNext:
    """the tower in torch bf16, channels_last: timm's op sequence (conv stem, LayerNorm over channels, depthwise conv, Linear MLP, layer scale)"""

    def __init__(self, arch, sd):
        self.arch = arch
        self.p = {k: v.to(DEV, torch.bfloat16) for k, v in sd.items() if k.startswith("visual.")}
        for k in list(self.p):
            if self.p[k].ndim == 4:
                self.p[k] = self.p[k].contiguous(memory_format=torch.channels_last)
        self.mean = torch.tensor(OPENAI_DATASET_MEAN, device=DEV).view(1, 3, 1, 1)
        self.std = torch.tensor(OPENAI_DATASET_STD, device=DEV).view(1, 3, 1, 1)

    def _ln_cl(self, x, name):   # x NCHW channels_last -> LayerNorm over C
        y = F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), self.p[name + ".weight"], self.p[name + ".bias"], self.arch.ln_eps)
        return y.permute(0, 3, 1, 2)

    @torch.no_grad()
    def __call__(self, u8):
        t, p, eps = "visual.trunk.", self.p, self.arch.ln_eps
        x = ((u8.permute(0, 3, 1, 2).float() / 255.0 - self.mean) / self.std).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x = self._ln_cl(F.conv2d(x, p[t + "stem.0.weight"], p[t + "stem.0.bias"], stride=4), t + "stem.1")
        for i, depth in enumerate(self.arch.depths):
            s = f"{t}stages.{i}."
            if i > 0:
                x = F.conv2d(self._ln_cl(x, s + "downsample.0"), p[s + "downsample.1.weight"], p[s + "downsample.1.bias"], stride=2)
            for j in range(depth):
                b = f"{s}blocks.{j}."
                C = x.shape[1]
                y = F.conv2d(x, p[b + "conv_dw.weight"], p[b + "conv_dw.bias"], padding=3, groups=C).permute(0, 2, 3, 1)
                y = F.layer_norm(y, (C,), p[b + "norm.weight"], p[b + "norm.bias"], eps)
                y = F.linear(F.gelu(F.linear(y, p[b + "mlp.fc1.weight"], p[b + "mlp.fc1.bias"])), p[b + "mlp.fc2.weight"], p[b + "mlp.fc2.bias"])
                x = x + (y * p[b + "gamma"]).permute(0, 3, 1, 2)
        pooled = F.layer_norm(x.mean((2, 3)), (x.shape[1],), p[t + "head.norm.weight"], p[t + "head.norm.bias"], eps)
        if self.arch.head == "linear":
            out = F.linear(pooled, p["visual.head.proj.weight"])
        else:
            out = F.linear(F.gelu(F.linear(pooled, p["visual.head.mlp.fc1.weight"], p["visual.head.mlp.fc1.bias"])), p["visual.head.mlp.fc2.weight"])
        return F.normalize(out.float(), dim=-1)


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default="convnext_base_w,convnext_large_d_320,convnext_xxlarge")
    ap.add_argument("--batches", default="64,128")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    for name in a.archs.split(","):
        v, _ = archs.resolve_open_clip(name)
        sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=0)
        tw = towers.ConvNextTower(v, sd, DEV)
        ref = None if a.no_torch else TorchConvNext(v, sd)
        for n in (int(b) for b in a.batches.split(",")):
            u8 = synthetic.natural_images_u8(n, v.image_size, v.image_size, seed=1).to(DEV)
            ms = time_ms(lambda: tw.encode_u8(u8), a.iters, a.warmup)
            gf = v.gflop_per_image * n
            row = {"arch": name, "image_size": v.image_size, "batch": n, "hip_ms": round(ms, 3), "hip_images_per_s": round(n / ms * 1e3, 1),
                   "gflop_per_image": round(v.gflop_per_image, 2), "hip_tflops": round(gf / ms, 1),
                   "hip_peak_frac": round(gf / ms / PEAK_BF16_TFLOPS, 3)}
            if ref is not None:
                tms = time_ms(lambda: ref(u8), a.iters, a.warmup)
                cos = float(F.cosine_similarity(tw.encode_u8(u8[:8]).double(), ref(u8[:8]).double(), dim=-1).min())
                row.update({"torch_bf16_ms": round(tms, 3), "torch_bf16_images_per_s": round(n / tms * 1e3, 1), "speedup_vs_torch": round(tms / ms, 2),
                            "min_cos_vs_torch_bf16": round(cos, 5)})
            print(json.dumps(row), flush=True)
        del tw, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
