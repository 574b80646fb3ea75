"""TEST INFRASTRUCTURE: the torch-CPU interpreter of ``tests/graph_interp.py`` extended by the two ops of YOLO11 graphs.

Same loop over the op list, the same un-packing of the blob (``graph_interp.unpack_conv`` / ``unpack_conv_h2``, ``h2_round``,
``act`` by import), plus the depthwise 3x3 and the PSA attention, evaluated from the blob exactly as ``csrc/yolo11_ops.hip``
reads it: depthwise weights [9][C] (tap ky * 3 + kx), the qkv slice as [q of all heads | k of all heads | v of all heads]."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from padel_analytics_amd import graph as G
from tests import graph_interp as GI
from tests.yolo11_ref import psa_attention


@torch.no_grad()
def run(graph: G.Graph, net_in: torch.Tensor, stale: float = 0.0):
    """net_in: (B, 3, H, W) fp32 in [0, 1] -> the list of buffers as NCHW tensors.  ``stale`` fills the buffers first: pad
    channels read under zero weights and never-written channels cannot leak into results."""
    blob = graph.blob()
    B, _, H, W = net_in.shape
    h2 = graph.dtype == G.DTYPE_H2
    assert graph.dtype != G.DTYPE_F16
    heads = set(graph.head_buf)
    bufs = [torch.full((B, c, H >> l, W >> l), float(stale)) for (l, c) in graph.bufs]

    def store(bi, lo, val):
        if h2 and bi not in heads:
            val = GI.h2_round(val)
        bufs[bi][:, lo:lo + val.shape[1]] = val

    def read(o, width=None):
        return bufs[o["in_buf"]][:, o["in_choff"]:o["in_choff"] + (o["cin"] if width is None else width)]

    for o in graph.ops:
        kd = o["kind"]
        if kd == G.OP_STEM:
            w = torch.from_numpy(blob[o["w_off"]:o["w_off"] + o["cout"] * 27].reshape(o["cout"], 3, 3, 3).transpose(0, 3, 1, 2).copy())
            b = torch.from_numpy(blob[o["b_off"]:o["b_off"] + o["cout"]].copy())
            store(o["out_buf"], o["out_choff"], F.silu(F.conv2d(net_in, w, b, stride=2, padding=1)))
        elif kd == G.OP_CONV:
            w, b = GI.unpack_conv_h2(blob, o) if h2 else GI.unpack_conv(blob, o)
            y = GI.act(F.conv2d(read(o), torch.from_numpy(w), torch.from_numpy(b.copy()), stride=o["stride"], padding=o["ksize"] // 2), o["act"])
            y = y[:, :o["cout"]]
            if o["res_buf"] >= 0:
                y = y + bufs[o["res_buf"]][:, o["res_choff"]:o["res_choff"] + o["cout"]]
            store(o["out_buf"], o["out_choff"], y)
        elif kd == G.OP_SPPF_POOL:
            c, t = o["cin"], bufs[o["in_buf"]]
            for k in range(3):
                src = t[:, o["in_choff"] + k * c:o["in_choff"] + (k + 1) * c]
                t[:, o["in_choff"] + (k + 1) * c:o["in_choff"] + (k + 2) * c] = F.max_pool2d(src, 5, 1, 2)
        elif kd == G.OP_UPSAMPLE2X:
            bufs[o["out_buf"]][:, o["out_choff"]:o["out_choff"] + o["cin"]] = F.interpolate(read(o), scale_factor=2.0, mode="nearest")
        elif kd == G.OP_DWCONV3:
            c = o["cin"]
            w = torch.from_numpy(blob[o["w_off"]:o["w_off"] + 9 * c].reshape(3, 3, c).transpose(2, 0, 1).copy())[:, None]
            b = torch.from_numpy(blob[o["b_off"]:o["b_off"] + c].copy())
            y = GI.act(F.conv2d(read(o), w, b, padding=1, groups=c), o["act"])
            if o["res_buf"] >= 0:
                y = y + bufs[o["res_buf"]][:, o["res_choff"]:o["res_choff"] + c]
            store(o["out_buf"], o["out_choff"], y)
        elif kd == G.OP_PSA_ATTN:
            nh, kk, hd = o["stride"], o["ksize"], o["npad"]
            x = read(o)
            Bx, _, h, w = x.shape
            q = x[:, :nh * kk].reshape(Bx, nh, kk, h * w)
            k = x[:, nh * kk:2 * nh * kk].reshape(Bx, nh, kk, h * w)
            v = x[:, 2 * nh * kk:].reshape(Bx, nh, hd, h * w)
            store(o["out_buf"], o["out_choff"], psa_attention(q, k, v, kk ** -0.5).reshape(Bx, nh * hd, h, w))
        else:
            raise AssertionError(kd)
    return bufs
