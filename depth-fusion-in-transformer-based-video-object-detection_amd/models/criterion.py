"""The training criterion (ref ``SetCriterion`` of models/deformable_detr_{single,multi,multi_plusplus}.py, the three are
the same): Hungarian assignment of every prediction set, then the classification, box and cardinality terms per set.

What the reference's loss computes, stated once:
  loss_ce            sum over all B*Q*3 logits of alpha_c * BCE(x, t) * (1 - p_t)^2 / num_boxes with alpha = (0, 1, 0.001)
                     as an fp32 table, t the one-hot of the matched label (none for unmatched rows) with column 2 REPLACED by
                     "column 1 is not 1"; ``focal_alpha`` is accepted and ignored, as the reference ignores it
  class_error        100 - top-1 accuracy of the matched rows (100 without any), last layer only
  loss_bbox          L1 of the matched boxes / num_boxes;   loss_giou  sum(1 - GIoU) of the matched pairs / num_boxes
  cardinality_error  mean over the images of | #(arg-max is not the last column) - T_b |, no gradient
  num_boxes          all targets of the batch, all-reduced and divided by the world size, at least 1
  aux_outputs[i]     the same under keys ``*_{i}`` (no class_error);  enc_outputs: against all-zero labels under ``*_enc``

Two routes.  fp32 predictions on the GPU: every set of the call goes through one launch each of ``dfx.ops.match_cost``,
``set_loss_forward`` and ``set_loss_backward`` (csrc/criterion.hip) with ONE host round trip for the assignment.  Anything
else - CPU tensors, other dtypes, a matcher that is not this project's, ``DFX_CRITERION=0`` - runs the op-by-op torch
formulation below, set after set, as the reference does.  Under CUDA graph capture the fused route raises.
"""
import torch
import torch.nn.functional as F
from torch import nn

from dfx import ops as _ops
from util import box_ops
from util.misc import get_world_size, is_dist_avail_and_initialized

from .matcher import HungarianMatcher, fused_route, refuse_capture, target_tensors

ALPHA_TABLE = (0.0, 1.0, 0.001)           # per-column weights of the classification loss (ref models/segmentation.py:222)
GAMMA = 2
LOSSES = ("labels", "cardinality", "boxes", "masks")

# Fused route: the shapes it was measured on and where it stands against the torch route are in
# profiles/r19_criterion.txt.  FUSED_MIN_ROWS: total prediction rows (B * sum of Q) from which the fused route is taken;
# 0 = always.
FUSED_MIN_ROWS = 0


class _Staging:
    """Pinned host buffers of one device, grown on demand, and the event that says the last call's copies have left them."""

    def __init__(self):
        self.desc = self.cost = self.row_target = None
        self.done = None

    def get(self, name, n, dtype):
        buf = getattr(self, name)
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(n, 1024), dtype=dtype).pin_memory()
            setattr(self, name, buf)
        return buf


class SetCriterion(nn.Module):
    """forward(outputs, targets) -> dict of losses with the reference's keys in the reference's order.  ``outputs``:
    pred_logits [B,Q,3], pred_boxes [B,Q,4] (cx, cy, w, h in 0..1), optionally aux_outputs (a list of such dicts, any Q)
    and enc_outputs; ``targets``: per image a dict with labels [T] int64 and boxes [T,4]."""

    def __init__(self, num_classes, matcher, weight_dict, losses, focal_alpha=0.25):
        super().__init__()
        if num_classes != len(ALPHA_TABLE):
            raise ValueError(f"SetCriterion: num_classes must be {len(ALPHA_TABLE)} - the reference's classification loss weights "
                             f"its columns by the three-column alpha table {list(ALPHA_TABLE)} and rewrites column 2 "
                             f"(modified_sigmoid_focal_loss); got num_classes={num_classes}")
        for loss in losses:
            assert loss in LOSSES, f"do you really want to compute {loss} loss?"
        if "masks" in losses:
            raise NotImplementedError("loss_masks: the segmentation head is outside this path")
        self.num_classes, self.matcher, self.weight_dict = num_classes, matcher, weight_dict
        self.losses, self.focal_alpha = list(losses), focal_alpha
        self._staging = {}

    # ---- what both routes share -------------------------------------------------------------------------------
    @staticmethod
    def _sets(outputs):
        """[(key suffix, set, labels all zero, with class_error)] in the reference's order"""
        sets = [("", {k: v for k, v in outputs.items() if k not in ("aux_outputs", "enc_outputs")}, False, True)]
        sets += [(f"_{i}", aux, False, False) for i, aux in enumerate(outputs.get("aux_outputs", ()))]
        if "enc_outputs" in outputs:
            sets.append(("_enc", outputs["enc_outputs"], True, False))
        return sets

    @staticmethod
    def _num_boxes(targets, device):
        count = sum(len(t["labels"]) for t in targets)
        if is_dist_avail_and_initialized():
            n = torch.as_tensor([count], dtype=torch.float, device=device)
            torch.distributed.all_reduce(n)
            return torch.clamp(n / get_world_size(), min=1).item()
        return max(float(count), 1.0)              # one process: no tensor, no synchronisation

    def _emit(self, losses, suffix, log, values):
        """values: loss_ce, class_error, loss_bbox, loss_giou, cardinality_error -> the keys of self.losses, in its order"""
        for loss in self.losses:
            if loss == "labels":
                losses["loss_ce" + suffix] = values[0]
                if log:
                    losses["class_error" + suffix] = values[1]
            elif loss == "cardinality":
                losses["cardinality_error" + suffix] = values[4]
            elif loss == "boxes":
                losses["loss_bbox" + suffix] = values[2]
                losses["loss_giou" + suffix] = values[3]

    def forward(self, outputs, targets):
        sets = self._sets(outputs)
        logits = outputs["pred_logits"]
        fused = (fused_route(logits) and type(self.matcher) is HungarianMatcher
                 and all(s["pred_logits"].dtype == torch.float32 and s["pred_logits"].device == logits.device for _, s, _, _ in sets)
                 and sum(s["pred_logits"].shape[0] * s["pred_logits"].shape[1] for _, s, _, _ in sets) >= FUSED_MIN_ROWS)
        return self._forward_fused(sets, targets) if fused else self._forward_torch(sets, targets)

    # ---- fused route ----------------------------------------------------------------------------------------------
    def assign(self, logits, boxes, labels, tboxes, desc_list, dims):
        """costs on the device -> pinned host memory -> every block solved -> (row_target on the device, descriptor on the device)"""
        S, B, rows, Ttot = dims
        dev = logits.device
        st = self._staging.setdefault(dev, _Staging())
        if st.done is not None:
            st.done.synchronize()                 # the previous call's copies out of the pinned buffers
        host_desc = st.get("desc", len(desc_list), torch.int32)
        host_desc[:len(desc_list)] = torch.tensor(desc_list, dtype=torch.int32)
        desc = torch.empty(len(desc_list), dtype=torch.int32, device=dev)
        desc.copy_(host_desc[:len(desc_list)], non_blocking=True)
        host_rt = st.get("row_target", rows, torch.int32)
        if Ttot:
            cost = _ops.match_cost(logits, boxes, labels, tboxes, desc, dims, self.matcher.cost_class, self.matcher.cost_bbox,
                                   self.matcher.cost_giou)
            host_cost = st.get("cost", cost.numel(), torch.float32)
            host_cost[:cost.numel()].copy_(cost, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()          # the one synchronisation of a criterion call
            _ops.lsap_ragged(host_cost, host_desc, dims, host_rt)
        else:
            host_rt[:rows].fill_(-1)
        row_target = torch.empty(rows, dtype=torch.int32, device=dev)
        row_target.copy_(host_rt[:rows], non_blocking=True)
        st.done = torch.cuda.Event()
        st.done.record(torch.cuda.current_stream(dev))
        return row_target, desc, host_rt[:rows]

    def _forward_fused(self, sets, targets):
        refuse_capture("SetCriterion")
        dev = sets[0][1]["pred_logits"].device
        B = sets[0][1]["pred_logits"].shape[0]
        labels, tboxes, counts = target_tensors(targets, dev)
        assert len(counts) == B, "one target dict per image"
        desc_list, dims = _ops.criterion_layout([s["pred_logits"].shape[1] for _, s, _, _ in sets], [z for _, _, z, _ in sets], counts)
        with torch.cuda.device(dev):
            logits = torch.cat([s["pred_logits"].reshape(-1, 3) for _, s, _, _ in sets]) if len(sets) > 1 else sets[0][1]["pred_logits"].reshape(-1, 3).contiguous()
            boxes = torch.cat([s["pred_boxes"].reshape(-1, 4) for _, s, _, _ in sets]) if len(sets) > 1 else sets[0][1]["pred_boxes"].reshape(-1, 4).contiguous()
            with torch.no_grad():
                row_target, desc, _ = self.assign(logits.detach(), boxes.detach(), labels, tboxes, desc_list, dims)
            out = _ops.SetLossFunction.apply(logits, boxes, labels, tboxes, row_target, desc, dims, 1.0 / self._num_boxes(targets, dev))
        values = out.flatten().unbind(0)
        losses = {}
        for i, (suffix, _, _, log) in enumerate(sets):
            v = values[5 * i:5 * i + 5]
            self._emit(losses, suffix, log, (v[0], v[1].detach(), v[2], v[3], v[4].detach()))
        return losses

    # ---- op-by-op torch route ---------------------------------------------------------------------------------------
    @staticmethod
    def _permutation(indices):
        batch = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        return batch, torch.cat([src for src, _ in indices])

    def _set_losses(self, logits, boxes, targets, indices, num_boxes):
        """-> loss_ce, class_error, loss_bbox, loss_giou, cardinality_error of one set, in the tensors' dtype.  Narrower
        dtypes than fp64 are evaluated in fp64 and rounded once at the end (values by the final cast, gradients by the cast's
        backward), as the kernels do: in fp32 the order of a sum decides the last bit of a loss, and the order differs between
        devices.  At these sizes the route is bound by its launches, not by the arithmetic."""
        out_dtype = logits.dtype
        if logits.is_floating_point() and out_dtype != torch.float64:
            logits, boxes = logits.double(), boxes.double()
            res = self._set_losses(logits, boxes, [{**t, "boxes": t["boxes"].double()} for t in targets], indices, num_boxes)
            return tuple(v.to(out_dtype) if i in (0, 2, 3) else v for i, v in enumerate(res))
        idx = self._permutation(indices)
        matched_labels = torch.cat([t["labels"][j] for t, (_, j) in zip(targets, indices)])
        classes = torch.full(logits.shape[:2], self.num_classes, dtype=torch.int64, device=logits.device)
        classes[idx] = matched_labels
        onehot = F.one_hot(classes, self.num_classes + 1)[..., :-1].to(logits.dtype)
        onehot = torch.cat([onehot[..., :2], (onehot[..., 1:2] != 1).to(logits.dtype)], dim=-1)
        prob = logits.sigmoid()
        ce = F.binary_cross_entropy_with_logits(logits, onehot, reduction="none")
        p_t = prob * onehot + (1 - prob) * (1 - onehot)
        alpha = torch.tensor(ALPHA_TABLE, device=logits.device)            # fp32, whatever the logits' dtype
        loss_ce = (alpha * (ce * (1 - p_t) ** GAMMA)).mean(1).sum() / num_boxes * logits.shape[1]

        with torch.no_grad():
            picked = logits[idx]
            if matched_labels.numel() == 0:
                class_error = 100 - torch.zeros([], device=logits.device)
            else:
                hits = (picked.argmax(-1) == matched_labels).float().sum()
                class_error = 100 - hits * (100.0 / matched_labels.numel())
            lengths = torch.as_tensor([len(t["labels"]) for t in targets], device=logits.device)
            card = (logits.argmax(-1) != logits.shape[-1] - 1).sum(1)
            cardinality = F.l1_loss(card.float(), lengths.float())

        src = boxes[idx]
        tgt = torch.cat([t["boxes"][j] for t, (_, j) in zip(targets, indices)], dim=0)
        loss_bbox = F.l1_loss(src, tgt, reduction="none").sum() / num_boxes
        giou = torch.diag(box_ops.generalized_box_iou(box_ops.box_cxcywh_to_xyxy(src), box_ops.box_cxcywh_to_xyxy(tgt)))
        loss_giou = (1 - giou).sum() / num_boxes
        return loss_ce, class_error, loss_bbox, loss_giou, cardinality

    def _forward_torch(self, sets, targets):
        num_boxes = self._num_boxes(targets, sets[0][1]["pred_logits"].device)
        losses = {}
        for suffix, s, zero, log in sets:
            tg = [{**t, "labels": torch.zeros_like(t["labels"])} for t in targets] if zero else targets
            indices = self.matcher(s, tg)
            self._emit(losses, suffix, log, self._set_losses(s["pred_logits"], s["pred_boxes"], tg, indices, num_boxes))
        return losses
