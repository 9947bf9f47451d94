"""Class-specific relevance maps of a compact model on MI355X: which patches speak for a given label.

``CompactAttributionViT`` is the inference twin of ``compact.CompactVisionTransformer`` that can also run a backward: the same flat
float32 parameter buffer, in the training layout and with the training shadows (the dgrads read the transposed weight copies), no
parameters, no gradient buffer, no optimizer hooks.  ``attribution`` goes through ``uvc_vit_compact_attribution`` (include/uvc_vit.h):
the training forward, the gradient of the chosen eval logit down to every block's attention output, and per attention block one
``uvc_attention_relevance_step`` -- the gradient-weighted attention rollout of Chefer, Gur & Wolf (ICCV 2021, "Generic Attention-Model
Explainability", self-attention rule).  ``compact.reference_attribution`` is its written spec.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import compact as CP

MAX_TOKENS = 256            # the attention backward at a value width (uvc_attention_bwd_vdim)


class CompactAttributionViT(CP._CompactModule):
    """``model(x)`` returns what ``CompactVisionTransformer`` returns (same kernels, same bits); ``model.attribution(x, target)`` adds
    the relevance map of one class per image."""

    def __init__(self, export: dict, precision: str = "bf16", device=None):
        super().__init__(export, precision, device, "uvc_vit_compact_train_layout", max_tokens=MAX_TOKENS)
        self.export = export
        dev = self._flat.device
        tsz = 4 if precision == "fp32" else 2
        self._shadow = torch.zeros(max(1, self._soff.n_total) * tsz, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(self._lib_call("uvc_vit_compact_train_update_shadows", L.ptr(self._flat), L.ptr(self._shadow), L.cur_stream()),
                    "uvc_vit_compact_train_update_shadows")
        self.eval()

    def forward(self, x=None, *, patches=None):
        """The eval forward, as ``CompactVisionTransformer.forward``: ``(eval logits, macs)``."""
        logits = self._eval_logits(x, patches)
        return logits, self.macs(logits.shape[0])

    def _targets(self, target, B, num_labels):
        """``target`` (an int, a sequence or a tensor of B indices) as an int32 device tensor [B], every index checked on the host."""
        dev = self._flat.device
        t = torch.as_tensor(target)
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError("target holds class indices (integers)")
        t = t.to(device="cpu", dtype=torch.int64).reshape(-1)
        if t.numel() == 1 and not isinstance(target, (list, tuple, torch.Tensor)):
            t = t.expand(B)
        if t.numel() != B:
            raise ValueError(f"{t.numel()} targets for a batch of {B} images")
        if int(t.min()) < 0 or int(t.max()) >= num_labels:
            raise ValueError(f"target must lie in [0, {num_labels}) (num_labels), not {t.tolist()}")
        return t.to(device=dev, dtype=torch.int32).contiguous()

    @torch.no_grad()
    def attribution(self, x=None, target=None, num_labels=None, *, patches=None):
        """``(eval logits, relevance, target)``: the logits are ``forward``'s bit for bit; ``relevance`` float32 [B, N] over the model's
        tokens (class, distillation, patches) is non-negative and NOT normalised (every row sums to at least 1, every readout entry is at
        least 1 / ntok; ``compact.reference_attribution`` is the spec); ``target`` int64 [B] is the class explained: the given one (an int,
        a sequence or a tensor of B indices), or with ``None`` the first maximum of the eval logits over the first ``num_labels`` columns
        (default: the model's num_classes).  Image batches only: patch rows are an eval-forward input."""
        if patches is not None:
            raise ValueError("patch rows stand in for the image batch of an eval forward: pass one of x / patches")
        nc = self._export["cfg"]["num_classes"]
        num_labels = nc if num_labels is None else int(num_labels)
        if not 1 <= num_labels <= nc:
            raise ValueError(f"num_labels {num_labels} must lie in [1, {nc}] (the model's head)")
        x = self._prep(x)
        B, dev = x.shape[0], self._flat.device
        given = None if target is None else self._targets(target, B, num_labels)
        self._refresh_shadows()
        io, mask = self._io(x, B, "attribution")
        logits = torch.empty(B, nc, device=dev)
        logits_dist = torch.empty(B, nc, device=dev) if self.num_tokens == 2 else None
        io.logits, io.logits_dist = L.ptr(logits), L.ptr(logits_dist)
        relevance = torch.empty(B, CP._seq(self._export["cfg"]), device=dev)
        chosen = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(self._lib_call("uvc_vit_compact_attribution", C.byref(io), L.ptr(given), num_labels, L.ptr(relevance), L.ptr(chosen), L.cur_stream()),
                "uvc_vit_compact_attribution")
        del mask, given                                  # (read by the launches above: alive until they are enqueued)
        return (logits if logits_dist is None else (logits + logits_dist) / 2), relevance, chosen.long()
