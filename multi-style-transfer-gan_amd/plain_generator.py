"""The plain CycleGAN ``Generator`` of the reference (pretrain.py:60-97 == batch_process_images.py:20-58 ==
gan_login_gui.py:168-205 == pretrain_resume.py:60-97) on the MI355X kernels.

Same ``Generator(channels=64)`` constructor, ``.encoder`` / ``.decoder`` ``nn.Sequential`` members with the reference's
child indices (state_dict keys ``encoder.{0,2,5,8}.*``, BatchNorm at ``encoder.{3,6,9}`` / ``decoder.{1,4,7}``,
``decoder.{0,3,6,9}.*``) and NCHW ``forward``.  Under data parallelism BatchNorm statistics are per rank (replicas
only) -- the reference never trains this class on more than one device either.

Inference fast path: ``half_inference()`` serves an eval-mode forward under ``torch.no_grad()`` from the fp16 kernels of
csrc/infer_f16_plain.hip with every BatchNorm folded into its convolution (mstg_hip/infer_plain.py); ``graph_inference()``
replays that forward from a captured hipGraph.  Training mode (batch statistics) and autograd keep the fp32 path below.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from mstg_hip.layers import HipBatchNorm2d, HipConv2d, HipConvTranspose2d, HipLeakyReLU, HipReLU, HipTanh
from mstg_hip.ops import ACT_LEAKY02, ACT_RELU, ACT_TANH
from mstg_hip import ops


class Generator(nn.Module):
    def __init__(self, channels=64):
        super().__init__()
        C = channels
        self.encoder = nn.Sequential(
            HipConv2d(3, C, 4, 2, 1), HipLeakyReLU(0.2),
            HipConv2d(C, C * 2, 4, 2, 1), HipBatchNorm2d(C * 2), HipLeakyReLU(0.2),
            HipConv2d(C * 2, C * 4, 4, 2, 1), HipBatchNorm2d(C * 4), HipLeakyReLU(0.2),
            HipConv2d(C * 4, C * 8, 4, 2, 1), HipBatchNorm2d(C * 8), HipLeakyReLU(0.2),
        )
        self.decoder = nn.Sequential(
            HipConvTranspose2d(C * 8, C * 4, 4, 2, 1), HipBatchNorm2d(C * 4), HipReLU(),
            HipConvTranspose2d(C * 4, C * 2, 4, 2, 1), HipBatchNorm2d(C * 2), HipReLU(),
            HipConvTranspose2d(C * 2, C, 4, 2, 1), HipBatchNorm2d(C), HipReLU(),
            HipConvTranspose2d(C, 3, 4, 2, 1), HipTanh(),
        )

    def half_inference(self, enable: bool = True):
        """Inference-only fast path: fp16 storage, fp16 MFMA, fp32 accumulation, BatchNorm (running statistics) folded into the
        convolutions' epilogues.  In eval mode under ``torch.no_grad()`` ``forward`` then returns an fp16 (N,3,H,W) tensor; in
        training mode, or with autograd enabled, the fp32 path still runs.  The packed filters are rebuilt lazily after a
        ``load_state_dict``; call ``half_inference()`` again after changing weights or running statistics in any other way."""
        if enable:  # fail here, not at the first forward
            from mstg_hip.infer_plain import check_width
            check_width(self.encoder[0].out_channels)
        self._half_enabled = bool(enable)
        self._half_plan = None
        if enable and not getattr(self, "_half_hook", False):
            self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_half_plan", None))
            self._half_hook = True
        return self

    def graph_inference(self, enable: bool = True):
        """Replay the inference forward (eval mode, under ``torch.no_grad()``) from a captured hipGraph, one per input shape: at
        batch 1 the launch gaps between the forward's dependent kernels cost more than the kernels.  The graph is re-captured
        after a ``load_state_dict``; the returned tensor is a copy of the graph's output buffer."""
        self._graph_enabled = bool(enable)
        self._graphs = {}
        if enable and not getattr(self, "_graph_hook", False):
            self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_graphs", {}))
            self._graph_hook = True
        return self

    def _inference(self):
        return not self.training and not torch.is_grad_enabled()

    def _half(self):
        if getattr(self, "_half_plan", None) is None:
            from mstg_hip.infer_plain import HalfPlainGeneratorPlan
            self._half_plan = HalfPlainGeneratorPlan(self)
        return self._half_plan

    def _graph_forward(self, x):
        key = (tuple(x.shape), x.dtype, bool(getattr(self, "_half_enabled", False)))
        entry = self._graphs.get(key)
        if entry is None:
            static_x = x.clone()
            for _ in range(2):  # warm-up outside the capture: lazy one-time set-up (kernel attributes, fp16 plan)
                self._forward_impl(static_x)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_y = self._forward_impl(static_x)
            entry = self._graphs[key] = (graph, static_x, static_y)
        graph, static_x, static_y = entry
        static_x.copy_(x)
        graph.replay()
        return static_y.clone()

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"Generator expects (N,3,H,W), got {tuple(x.shape)}")
        if x.shape[2] % 16 or x.shape[3] % 16:
            raise RuntimeError(f"Generator: H and W must be multiples of 16 (four stride-2 stages), got {x.shape[2]}x{x.shape[3]}")
        if getattr(self, "_graph_enabled", False) and self._inference() and x.is_cuda:
            return self._graph_forward(x.contiguous())
        return self._forward_impl(x)

    def _forward_impl(self, x):
        if getattr(self, "_half_enabled", False) and self._inference():
            return self._half().forward(x)
        e, d = self.encoder, self.decoder
        h = ops.activation(e[0](x, nhwc=True, x_nchw=True), ACT_LEAKY02)
        for ci, bi in ((2, 3), (5, 6), (8, 9)):
            h = e[bi](e[ci](h, nhwc=True), nhwc=True, act=ACT_LEAKY02)
        for ci, bi in ((0, 1), (3, 4), (6, 7)):
            h = d[bi](d[ci](h, nhwc=True), nhwc=True, act=ACT_RELU)
        return d[9](h, nhwc=True, y_nchw=True, act=ACT_TANH)
