"""fp64 restatement of the multi-scale detection backbone (DINO ``models/dino/fastervit.py`` = DET), functional over a state_dict.

TEST INFRASTRUCTURE ONLY.  Written in this repository from the reference's semantics; the conv side and the attention / MLP / LayerNorm
pieces that the detection variant shares with the classifier come from the frozen classifier oracle (``oracle/``).  What is restated here
is what the detection variant does differently:

* TokenInitializer (DET:569-592): pool kernel / stride from the padded map, zero pad to a multiple of ct_size, raw NCHW reshape;
* rank-2 PosEmbMLPSwinv1D.forward(x, h_g, w_g) (DET:176-203): arange(h_g) x arange(w_g), normalised by (token count) // 2;
* HAT.forward (DET:498-540) with carrier tokens travelling as (ct, hg, wg) and a carrier attention bias padded or cropped to G;
* FasterViTLayer.forward (DET:686-708): pad, crop, and the pre-downsample map as the level output; ``norm{i}`` as eval BatchNorm2d.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle import hat_reference as hr
from oracle import model_reference as mr

Tensor = torch.Tensor
SD = Dict[str, Tensor]


def pos_grid(sd: SD, prefix: str, h: int, w: int, dtype) -> Tensor:
    """(1, h*w, C): the position MLP over the raster grid arange(h) x arange(w), shifted and divided by (h*w) // 2."""
    n = h * w
    dev = sd[prefix + "cpb_mlp.0.weight"].device
    ys = torch.arange(h, dtype=dtype, device=dev)
    xs = torch.arange(w, dtype=dtype, device=dev)
    grid = torch.stack(torch.meshgrid(ys, xs, indexing="ij")).reshape(2, n).t().unsqueeze(0)
    grid = (grid - n // 2) / (n // 2)
    w0 = sd[prefix + "cpb_mlp.0.weight"].to(dtype)
    b0 = sd[prefix + "cpb_mlp.0.bias"].to(dtype)
    w2 = sd[prefix + "cpb_mlp.2.weight"].to(dtype)
    return F.linear(torch.relu(F.linear(grid, w0, b0)), w2)


def attention(x: Tensor, sd: SD, prefix: str, heads: int, res: int) -> Tensor:
    """WindowAttention.forward (DET:393-404) on any device: oracle.hat_reference.window_attention with the bias table evaluated on the CPU
    (the oracle builds its coordinate tables there) and moved to x's device.  The bias is built for res^2 tokens and F.pad-ed by
    S - res^2 on the top / left: zero rows / columns for S > res^2, a crop for S < res^2."""
    dtype = x.dtype
    Bw, S, C = x.shape
    d = C // heads
    pre = prefix + "pos_emb_funct."
    cpu = {pre + k: sd[pre + k].cpu() for k in ("cpb_mlp.0.weight", "cpb_mlp.0.bias", "cpb_mlp.2.weight")}
    bias = hr.attn_bias(cpu, pre, res, heads, S, dtype).to(x.device)
    qkv = F.linear(x, sd[prefix + "qkv.weight"].to(dtype), sd[prefix + "qkv.bias"].to(dtype))
    q, k, v = qkv.reshape(Bw, -1, 3, heads, d).permute(2, 0, 3, 1, 4)
    a = ((q @ k.transpose(-2, -1)) * d ** -0.5 + bias.unsqueeze(0)).softmax(dim=-1)
    out = (a @ v).transpose(1, 2).reshape(Bw, -1, C)
    return F.linear(out, sd[prefix + "proj.weight"].to(dtype), sd[prefix + "proj.bias"].to(dtype))


def pool_geometry(Hp: int, Wp: int, ws: int, cw: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((kh, kw), (sh, sw)) of the carrier-token average pool for a padded Hp x Wp map."""
    ks, ss = [], []
    for r in (Hp, Wp):
        o = int(cw * r / ws)
        s = int(r / o)
        ks.append(r - (o - 1) * s)
        ss.append(s)
    return (ks[0], ks[1]), (ss[0], ss[1])


def token_init(x: Tensor, sd: SD, prefix: str, ws: int, cw: int) -> Tuple[Tensor, int, int]:
    """(B, G, C) carrier tokens in raw memory order of the pooled NCHW map, and the carrier grid (hg, wg)."""
    B, C, Hp, Wp = x.shape
    k, s = pool_geometry(Hp, Wp, ws, cw)
    y = F.conv2d(x, sd[prefix + "pos_embed.weight"].to(x.dtype), sd[prefix + "pos_embed.bias"].to(x.dtype), padding=1, groups=C)
    y = F.avg_pool2d(y, kernel_size=k, stride=s)
    H, W = y.shape[2], y.shape[3]
    y = F.pad(y, (0, (cw - W % cw) % cw, 0, (cw - H % cw) % cw))
    hg, wg = y.shape[2], y.shape[3]
    return y.reshape(B, hg * wg, C), hg, wg


def hat_block(x: Tensor, ct: Optional[Tensor], hg: int, wg: int, sd: SD, prefix: str, *, heads: int, ws: int, cw: int, hier: bool,
              hat_res: int, last: bool, do_propagation: bool) -> Tuple[Tensor, Optional[Tensor]]:
    dtype = x.dtype
    Bw, _, C = x.shape
    x = x + pos_grid(sd, prefix + "pos_embed.", ws, ws, dtype)
    if hier:
        Bg, Ng, Hg = ct.shape
        ct = hr.ct_dewindow(ct, hg, wg, cw)
        ct = ct + pos_grid(sd, prefix + "hat_pos_embed.", hg, wg, dtype)
        g1 = hr._gamma(sd, prefix + "gamma1", dtype)
        g2 = hr._gamma(sd, prefix + "gamma2", dtype)
        # the bias is built for hat_res^2 tokens and padded (G larger) or cropped (G smaller) to the G carrier tokens
        ct = ct + g1 * attention(hr.layer_norm(ct, sd, prefix + "hat_norm1."), sd, prefix + "hat_attn.", heads, hat_res)
        ct = ct + g2 * hr.mlp(hr.layer_norm(ct, sd, prefix + "hat_norm2."), sd, prefix + "hat_mlp.")
        ct = hr.ct_window(ct, hg, wg, cw).reshape(Bw, -1, C)
        x = torch.cat((ct, x), dim=1)
    g3 = hr._gamma(sd, prefix + "gamma3", dtype)
    g4 = hr._gamma(sd, prefix + "gamma4", dtype)
    x = x + g3 * attention(hr.layer_norm(x, sd, prefix + "norm1."), sd, prefix + "attn.", heads, ws)
    x = x + g4 * hr.mlp(hr.layer_norm(x, sd, prefix + "norm2."), sd, prefix + "mlp.")
    if hier:
        ctr, x = x.split([x.shape[1] - ws * ws, ws * ws], dim=1)
        ct = ctr.reshape(Bg, Ng, Hg)
        if last and do_propagation:
            img = ctr.transpose(1, 2).reshape(Bw, C, cw, cw)
            x = x + g1 * F.interpolate(img, size=(ws, ws), mode="nearest").flatten(2).transpose(1, 2)
    return x, ct


def transformer_level(x: Tensor, sd: SD, prefix: str, *, depth: int, heads: int, ws: int, cw: int, input_resolution: int, only_local: bool,
                      do_propagation: bool) -> Tensor:
    """Transformer branch of the level, pre-downsample output (cropped to the input size)."""
    B, C, H, W = x.shape
    sr_build = 1 if only_local else input_resolution // ws
    hier = sr_build > 1
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    if pad_r or pad_b:
        x = F.pad(x, (0, pad_r, 0, pad_b))
    Hp, Wp = x.shape[2], x.shape[3]
    ct, hg, wg = (None, 0, 0)
    if hier and depth > 0:
        ct, hg, wg = token_init(x, sd, prefix + "global_tokenizer.", ws, cw)
    hat_res = int((cw * cw * sr_build * sr_build) ** 0.5)
    x = hr.window_partition(x, ws)
    for i in range(depth):
        x, ct = hat_block(x, ct, hg, wg, sd, f"{prefix}blocks.{i}.", heads=heads, ws=ws, cw=cw, hier=hier, hat_res=hat_res,
                          last=(i == depth - 1), do_propagation=do_propagation)
    x = hr.window_reverse(x, ws, Hp, Wp, B)
    return x[:, :, :H, :W]


def backbone_forward(sd: SD, x: Tensor, cfg: dict, out_indices: Sequence[int] = (0, 1, 2, 3), resolution: int = 224,
                     dtype=torch.float64) -> Tuple[Tensor, ...]:
    """Normalised pre-downsample maps of the ``out_indices`` levels (NCHW, ``dtype``).  ``cfg``: the builder's configuration (depths,
    num_heads, window_size, ct_size, hat, do_propagation)."""
    x = mr.patch_embed(x.to(dtype), sd)
    hat = cfg.get("hat") or [True] * len(cfg["depths"])
    outs = []
    for i, depth in enumerate(cfg["depths"]):
        prefix = f"levels.{i}."
        if i < 2:
            # DET:687-704 pads EVERY level to a multiple of its window, the conv levels too: the 3x3 convs then see the padded zeros
            # and the second conv sees the first conv's values in the pad, not its implicit zero padding, near the right / bottom edge
            H, W = x.shape[2], x.shape[3]
            ws = cfg["window_size"][i]
            x = F.pad(x, (0, (ws - W % ws) % ws, 0, (ws - H % ws) % ws))
            for b in range(depth):
                x = mr.conv_block(x, sd, f"{prefix}blocks.{b}.")
            xo = x[:, :, :H, :W]
        else:
            xo = transformer_level(x, sd, prefix, depth=depth, heads=cfg["num_heads"][i], ws=cfg["window_size"][i], cw=cfg["ct_size"],
                                   input_resolution=int(2 ** (-2 - i) * resolution), only_local=not hat[i],
                                   do_propagation=bool(cfg.get("do_propagation", False)))
        x = mr.downsample(xo, sd, prefix + "downsample.") if i < 3 else xo
        if i in out_indices:
            outs.append(mr._bn(xo, sd, f"norm{i}.", 1e-5))
    return tuple(outs)
