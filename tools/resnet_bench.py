"""ResNet CLIP image towers: images/s of the HIP tower (one mq_encode_resnet_u8 call per batch) against the same tower written in torch bf16,
channels_last (F.conv2d / F.multi_head_attention_forward: MIOpen / hipBLASLt — how open_clip runs it), both in this process, from resident uint8 images,
timed with device events after warm-up.  The torch tower is a yardstick only; it is never on the product path.

  python tools/resnet_bench.py [--archs RN50,RN50x16] [--batches 64,256] [--iters 10] [--no-torch]

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


class TorchResNet:
    """the tower in torch bf16, channels_last: ModifiedResNet's op sequence (conv, eval BatchNorm, ReLU, avg-pool strides, attention pool)"""

    def __init__(self, arch, sd):
        self.arch = arch
        self.p = {k: v.to(DEV, torch.bfloat16) for k, v in sd.items() if k.startswith("visual.") and v.is_floating_point()}
        for k in list(self.p):
            if self.p[k].ndim == 4:
                self.p[k] = self.p[k].contiguous(memory_format=torch.channels_last)
        self.mean = torch.tensor(OPENAI_DATASET_MEAN, device=DEV).view(1, 3, 1, 1)
        self.std = torch.tensor(OPENAI_DATASET_STD, device=DEV).view(1, 3, 1, 1)

    def _bn(self, x, n):
        p = self.p
        return F.batch_norm(x, p[n + ".running_mean"], p[n + ".running_var"], p[n + ".weight"], p[n + ".bias"], False, 0.0, 1e-5)

    @torch.no_grad()
    def __call__(self, u8):
        p, v = self.p, "visual."
        x = ((u8.permute(0, 3, 1, 2).float() / 255.0 - self.mean) / self.std).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x = F.relu(self._bn(F.conv2d(x, p[v + "conv1.weight"], stride=2, padding=1), v + "bn1"))
        x = F.relu(self._bn(F.conv2d(x, p[v + "conv2.weight"], padding=1), v + "bn2"))
        x = F.avg_pool2d(F.relu(self._bn(F.conv2d(x, p[v + "conv3.weight"], padding=1), v + "bn3")), 2)
        for i, depth in enumerate(self.arch.layers):
            for j in range(depth):
                b = f"{v}layer{i + 1}.{j}."
                stride = 2 if (i > 0 and j == 0) else 1
                out = F.relu(self._bn(F.conv2d(x, p[b + "conv1.weight"]), b + "bn1"))
                out = F.relu(self._bn(F.conv2d(out, p[b + "conv2.weight"], padding=1), b + "bn2"))
                if stride > 1:
                    out = F.avg_pool2d(out, stride)
                out = self._bn(F.conv2d(out, p[b + "conv3.weight"]), b + "bn3")
                idn = x
                if b + "downsample.0.weight" in p:
                    idn = self._bn(F.conv2d(F.avg_pool2d(x, stride) if stride > 1 else x, p[b + "downsample.0.weight"]), b + "downsample.1")
                x = F.relu(out + idn)
        C = x.shape[1]
        t = x.flatten(2).permute(2, 0, 1)
        t = torch.cat([t.mean(0, keepdim=True), t]) + p[v + "attnpool.positional_embedding"][:, None, :]
        a = v + "attnpool."
        out, _ = F.multi_head_attention_forward(
            query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=C // 64, q_proj_weight=p[a + "q_proj.weight"],
            k_proj_weight=p[a + "k_proj.weight"], v_proj_weight=p[a + "v_proj.weight"], in_proj_weight=None,
            in_proj_bias=torch.cat([p[a + "q_proj.bias"], p[a + "k_proj.bias"], p[a + "v_proj.bias"]]), bias_k=None, bias_v=None,
            add_zero_attn=False, dropout_p=0.0, out_proj_weight=p[a + "c_proj.weight"], out_proj_bias=p[a + "c_proj.bias"],
            use_separate_proj_weight=True, training=False, need_weights=False)
        return F.normalize(out[0].float(), dim=-1)


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
    ap.add_argument("--archs", default="RN50,RN50x16")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    for name in a.archs.split(","):
        v, _ = archs.resolve_resnet_clip(name)
        sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=0)
        tw = towers.ResNetTower(v, sd, DEV)
        ref = None if a.no_torch else TorchResNet(v, sd)
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
