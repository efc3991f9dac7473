"""Hungarian matching between predictions and targets (ref models/matcher.py): ``HungarianMatcher``, ``build_matcher``.

The cost of a (query, target) pair is  cost_bbox * L1 + cost_class * focal cost + cost_giou * (-GIoU)  with the focal cost's
alpha = 0.25 and gamma = 2 fixed, as in the reference; only the pairs of an image with its own targets are ever solved.
fp32 predictions on the GPU get their costs from one launch of ``dfx.ops.match_cost``; anything else (CPU tensors, other
dtypes, ``DFX_CRITERION=0``) from the op-by-op torch formulation below.  The assignment itself runs on the host in both
routes, by the library's own solver (``dfx.ops.lsap``): there is no scipy on this path.
"""
import os

import torch
from torch import nn

from dfx import ops as _ops
from util.box_ops import box_cxcywh_to_xyxy, generalized_box_iou

FOCAL_ALPHA, FOCAL_GAMMA = 0.25, 2.0          # of the matching cost (ref models/matcher.py:78-79)


def fused_route(t):
    """fp32 on the GPU and not switched off: the criterion's kernels serve this tensor."""
    return t.is_cuda and t.dtype == torch.float32 and os.environ.get("DFX_CRITERION", "1") != "0"


def refuse_capture(what):
    """The assignment is a host round trip (costs to the host, solve, row targets back): it cannot be captured."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} cannot run under CUDA graph capture: the Hungarian assignment is solved on the host "
                           "(one stream synchronisation per call); capture the model and run the criterion outside the graph")


def target_tensors(targets, device, zero_labels=False):
    """-> (labels [Ttot] int32, boxes [Ttot,4] fp32, counts per image) on ``device``"""
    counts = [int(t["labels"].shape[0]) for t in targets]
    if sum(counts) == 0:
        return (torch.empty(0, dtype=torch.int32, device=device), torch.empty((0, 4), dtype=torch.float32, device=device), counts)
    labels = torch.cat([t["labels"] for t in targets]).to(device=device, dtype=torch.int32)
    boxes = torch.cat([t["boxes"] for t in targets]).to(device=device, dtype=torch.float32).contiguous()
    return (torch.zeros_like(labels) if zero_labels else labels), boxes, counts


class HungarianMatcher(nn.Module):
    """forward(outputs, targets) -> [(index_i, index_j)] per image: int64 CPU tensors of min(num_queries, num_targets)
    matched (query, target) indices, sorted by query  (ref models/matcher.py:20-100)."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1):
        super().__init__()
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"

    def cost_matrix(self, logits, boxes, tgt_ids, tgt_bbox):
        """[B*Q, Ttot] costs of every prediction against every target of the batch, op by op in the tensors' dtype"""
        prob = logits.flatten(0, 1).sigmoid()
        out_bbox = boxes.flatten(0, 1)
        neg = (1 - FOCAL_ALPHA) * (prob ** FOCAL_GAMMA) * (-(1 - prob + 1e-8).log())
        pos = FOCAL_ALPHA * ((1 - prob) ** FOCAL_GAMMA) * (-(prob + 1e-8).log())
        cost_class = pos[:, tgt_ids] - neg[:, tgt_ids]
        cost_bbox = torch.cdist(out_bbox, tgt_bbox, p=1)
        cost_giou = -generalized_box_iou(box_cxcywh_to_xyxy(out_bbox), box_cxcywh_to_xyxy(tgt_bbox))
        return self.cost_bbox * cost_bbox + self.cost_class * cost_class + self.cost_giou * cost_giou

    @torch.no_grad()
    def forward(self, outputs, targets):
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        B, Q = logits.shape[:2]
        counts = [int(t["boxes"].shape[0]) for t in targets]
        if fused_route(logits) and logits.shape[-1] == 3:
            refuse_capture("HungarianMatcher")
            labels, tboxes, counts = target_tensors(targets, logits.device)
            desc, dims = _ops.criterion_layout([Q], [False], counts)
            cost = _ops.match_cost(logits.reshape(-1, 3).contiguous(), boxes.reshape(-1, 4).contiguous(), labels, tboxes,
                                   torch.tensor(desc, dtype=torch.int32).to(logits.device), dims,
                                   self.cost_class, self.cost_bbox, self.cost_giou).cpu()
            off = desc[3:]
            blocks = [cost[Q * off[b]:Q * off[b + 1]].view(Q, counts[b]) for b in range(B)]
        else:
            tgt_ids = torch.cat([t["labels"] for t in targets])
            tgt_bbox = torch.cat([t["boxes"] for t in targets])
            C = self.cost_matrix(logits, boxes, tgt_ids, tgt_bbox).view(B, Q, -1).cpu()
            blocks = [c[b] for b, c in enumerate(C.split(counts, -1))]
        return [_ops.lsap(block) for block in blocks]


def build_matcher(args):
    return HungarianMatcher(cost_class=args.set_cost_class, cost_bbox=args.set_cost_bbox, cost_giou=args.set_cost_giou)
