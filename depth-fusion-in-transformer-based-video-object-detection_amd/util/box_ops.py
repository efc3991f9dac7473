"""Box helpers on the inference path (ref util/box_ops.py:17-28)."""
import torch


def box_cxcywh_to_xyxy(x):
    cx, cy, w, h = x.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def box_xyxy_to_cxcywh(x):
    x0, y0, x1, y1 = x.unbind(-1)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], dim=-1)


def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def box_iou(boxes1, boxes2):
    """Pairwise IoU of xyxy boxes [N,4] x [M,4] -> (iou [N,M], union [N,M])  (ref util/box_ops.py:32-45)."""
    area1, area2 = box_area(boxes1), box_area(boxes2)
    wh = (torch.min(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, None, :2], boxes2[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2 - inter
    return inter / union, union


def generalized_box_iou(boxes1, boxes2):
    """Pairwise GIoU of xyxy boxes [N,4] x [M,4] -> [N,M]; boxes with x1 < x0 or y1 < y0 are refused, as the reference
    refuses them (ref util/box_ops.py:48-69)."""
    assert (boxes1[:, 2:] >= boxes1[:, :2]).all() and (boxes2[:, 2:] >= boxes2[:, :2]).all(), "degenerate boxes"
    iou, union = box_iou(boxes1, boxes2)
    wh = (torch.max(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.min(boxes1[:, None, :2], boxes2[:, :2])).clamp(min=0)
    area = wh[..., 0] * wh[..., 1]
    return iou - (area - union) / area
