"""RoIAlign backward: the reference the tests rest on, and their input builders (helper module, no fixtures).

``roi_align_torch`` restates csrc/roi_align.hip (``load_roi`` / ``locate``) in differentiable torch: the index
arithmetic runs in fp32 exactly as in the kernels (same expressions, same order), the values are gathered in
``x.dtype``.  Autograd through it in fp64 is the backward reference - the oracle has no RoIAlign backward.
tests/test_roi_backward_cpu.py pins its forward to ``oracle.roi_align``.
"""
import torch

# the RoI list of tests/test_models_gpu.py::test_roi_align_kernels_match_oracle, a RoI wholly off the map and one that
# hangs over the bottom-right corner (image 416 x 672 at scale 1/32 = map 13 x 21)
LIST_ROIS = [[0, 10., 12., 200., 150.], [1, -20., -5., 100., 400.], [0, 300., 100., 340., 140.],
             [1, 50., 60., 50.5, 60.5], [0, 0., 0., 672., 416.], [1, -100., -100., -40., -50.],
             [0, 600., 380., 900., 700.]]


def _pair(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def sample_coords(rois, size, scale, sr, aligned=True):
    """fp32 sample coordinates as the kernels compute them: ys [K,ph,sr], xs [K,pw,sr], batch index [K]."""
    ph, pw = _pair(size)
    r = rois.detach().float()
    scale = torch.tensor(scale, dtype=torch.float32)
    off = 0.5 if aligned else 0.0
    b = r[:, 0].long()
    x1 = r[:, 1] * scale - off
    y1 = r[:, 2] * scale - off
    rw = r[:, 3] * scale - off - x1
    rh = r[:, 4] * scale - off - y1
    if not aligned:
        rw, rh = rw.clamp(min=1.0), rh.clamp(min=1.0)
    bw, bh = rw / pw, rh / ph
    s = torch.arange(sr, dtype=torch.float32)
    i = torch.arange(ph, dtype=torch.float32)
    j = torch.arange(pw, dtype=torch.float32)
    ys = y1[:, None, None] + i[None, :, None] * bh[:, None, None] + (s[None, None, :] + 0.5) * bh[:, None, None] / sr
    xs = x1[:, None, None] + j[None, :, None] * bw[:, None, None] + (s[None, None, :] + 0.5) * bw[:, None, None] / sr
    return ys, xs, b


def _axis(v, n):
    """``locate`` along one axis: valid, low index, high index, low fraction, high fraction."""
    ok = ~((v < -1.0) | (v > n))
    v = v.clamp(min=0.0)
    lo = v.clamp(max=float(n)).long()
    top = lo >= n - 1
    lo = torch.where(top, torch.full_like(lo, n - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    v = torch.where(top, lo.float(), v)
    frac = v - lo.float()
    return ok, lo, hi, frac, 1.0 - frac


def roi_align_torch(x, rois, size, scale, sr, aligned=True, hits=False):
    """x [N,C,H,W] (any float dtype), rois [K,5] -> [K,C,ph,pw]; differentiable in x only (the RoIs are detached, as
    the operator gives them no gradient).  A RoI whose batch index is outside [0, N) pools zeros.
    ``hits=True`` replaces every corner weight of a valid sample by 1 and drops the 1/sr^2: the backward of that
    map counts (RoI, bin, sample, corner) hits per pixel."""
    N, C, H, W = x.shape
    K = rois.shape[0]
    ph, pw = _pair(size)
    ys, xs, b = sample_coords(rois, size, scale, sr, aligned)
    live = (b >= 0) & (b < N)
    oky, yl, yh, ly, hy = _axis(ys, H)
    okx, xl, xh, lx, hx = _axis(xs, W)
    flat = x[b.clamp(0, N - 1)].reshape(K, C, H * W)
    ok = (oky[:, :, :, None, None] & okx[:, None, None, :, :] & live[:, None, None, None, None]).to(x.dtype)
    out = x.new_zeros(K, C, ph, sr, pw, sr)
    for yy, wy in ((yl, hy), (yh, ly)):
        for xx, wx in ((xl, hx), (xh, lx)):
            idx = (yy[:, :, :, None, None] * W + xx[:, None, None, :, :]).reshape(K, 1, -1).expand(-1, C, -1)
            w = ok if hits else (wy[:, :, :, None, None] * wx[:, None, None, :, :]).to(x.dtype) * ok
            out = out + torch.gather(flat, 2, idx).view(K, C, ph, sr, pw, sr) * w[:, None]
    out = out.sum((3, 5))
    return out if hits else out / (sr * sr)


def roi_align_like_ops(inp, rois, output_size, spatial_scale, sampling_ratio, aligned=True, channels_last=False):
    """The restatement behind the signature of ``dfx.ops.roi_align`` (any device, any float dtype)."""
    if channels_last:
        out = roi_align_torch(inp.permute(0, 3, 1, 2), rois, output_size, spatial_scale, sampling_ratio, aligned)
        return out.flatten(2).transpose(1, 2).contiguous()
    return roi_align_torch(inp, rois, output_size, spatial_scale, sampling_ratio, aligned)


def reference_backward(shape, rois, grad_out, size, scale, sr, aligned=True, hits=False, chunk=64):
    """d<roi_align_torch(x), grad_out>/dx in fp64 for x of ``shape`` [N,C,H,W] (the map is linear in x, so x = 0
    serves), RoIs in chunks to bound memory."""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    g = grad_out.double()
    for k in range(0, rois.shape[0], chunk):
        roi_align_torch(x, rois[k:k + chunk], size, scale, sr, aligned, hits).backward(g[k:k + chunk])
    return x.grad if x.grad is not None else torch.zeros(shape, dtype=torch.float64)


def random_rois(n_images, per_image, img_h, img_w, seed):
    """Boxes with centres uniform over the image widened by 10 % a side and sides 1/16 .. 1/2 of the image's."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(n_images):
        cx = (torch.rand(per_image, generator=g) * 1.2 - 0.1) * img_w
        cy = (torch.rand(per_image, generator=g) * 1.2 - 0.1) * img_h
        w = (1 / 16 + torch.rand(per_image, generator=g) * (1 / 2 - 1 / 16)) * img_w
        h = (1 / 16 + torch.rand(per_image, generator=g) * (1 / 2 - 1 / 16)) * img_h
        rows.append(torch.stack([torch.full((per_image,), float(b)), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1))
    return torch.cat(rows)


def drop_near_skip_bounds(rois, H, W, size, scale, sr, aligned, margin=1e-3):
    """Drop every box with a sample coordinate within ``margin`` of a bound of the skip rule (-1, H for y; -1, W
    for x): the rule is discontinuous there and the kernels may contract the coordinate arithmetic with FMAs where
    torch does not.  Returns (kept RoIs, share dropped)."""
    ys, xs, _ = sample_coords(rois, size, scale, sr, aligned)
    near = lambda v, n: (((v + 1.0).abs() < margin) | ((v - n).abs() < margin)).flatten(1).any(1)
    bad = near(ys, float(H)) | near(xs, float(W))
    return rois[~bad], bad.float().mean().item()


def random_family(H, W, aligned, sr, seed, per_image=300, n_images=2, size=7, scale=1 / 32):
    """Family (b): the list plus ``per_image`` random boxes per image on an H x W map of a (H/scale) x (W/scale) image."""
    rois = torch.cat([torch.tensor(LIST_ROIS), random_rois(n_images, per_image, H / scale, W / scale, seed)])
    kept, dropped = drop_near_skip_bounds(rois, H, W, size, scale, sr, aligned)
    assert dropped <= 0.02, f"the skip-bound filter dropped {dropped:.1%} of the boxes (at most 2 % allowed)"
    return kept


def random_bound(shape, rois, grad_out, size, scale, sr, aligned):
    """Reference and elementwise bound of family (b) for grad_input [N,C,H,W] (tests/test_roi_backward_gpu.py):
    |got - ref64| <= (n + 8) * 2^-24 * mag + 16 * 2^-24 * max(H, W) * G."""
    H, W = shape[2], shape[3]
    ref = reference_backward(shape, rois, grad_out, size, scale, sr, aligned)
    mag = reference_backward(shape, rois, grad_out.abs(), size, scale, sr, aligned)
    n = reference_backward((shape[0], 1, H, W), rois, torch.ones(rois.shape[0], 1, *_pair(size)), size, scale, sr,
                           aligned, hits=True)
    G = reference_backward(shape, rois, grad_out.abs() / (sr * sr), size, scale, sr, aligned, hits=True)
    G = torch.nn.functional.max_pool2d(G, 3, stride=1, padding=1)       # a vanishing weight may land on a neighbour
    eps = 2.0 ** -24
    return ref, (n + 8) * eps * mag + 16 * eps * max(H, W) * G


# ---- family (a): every product and partial sum exactly representable -----------------------------------------
EXACT_SCALE, EXACT_SIZE, EXACT_SR = 1 / 32, 7, 2


def exact_family(N=2, C=68, H=16, W=32, K=64, seed=9):
    """scale 1/32, aligned, sr 2, 7 x 7 bins; x1*scale - 0.5 and y1*scale - 0.5 multiples of 1/8 from -2 to the map
    size; box sides on the map 7*m/4, m in 1..8: bin m/4, sample step m/8, first sample m/16 into the bin, so every
    coordinate is a multiple of 1/16 and every corner weight a multiple of 2^-8; values k/8, grad_out k/4 with
    |k| <= 4.  Terms into one grad_input element are multiples of 2^-12 (2^-8 * 1/4 * 2^-2); with their magnitudes
    summing to less than 2^12 every partial sum in any order is an fp32 number (24 bits), so the atomics' arrival
    order cannot matter.  (Counting the half-step offset makes the grid 1/16 and the budget 2^12, not the 1/8 and 2^14
    of a first estimate; the family's largest sum of magnitudes is about 12.)  Returns x [N,C,H,W], rois, grad_out."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    rows = []
    for k in range(K):
        m, mh = ri(1, 9), ri(1, 9)
        sx, sy = ri(-16, 8 * W) / 8.0, ri(-16, 8 * H) / 8.0            # x1*scale - 0.5, y1*scale - 0.5
        rows.append([k % N, (sx + 0.5) * 32, (sy + 0.5) * 32, (sx + 7 * m / 4 + 0.5) * 32, (sy + 7 * mh / 4 + 0.5) * 32])
    # the edges the family must hold whatever the draw: a start before the map with samples below -1 (skipped) and in
    # [-1, 0] (clamped), an end beyond the map, batch indices outside [0, N)
    rows[0] = [0, (-2 + 0.5) * 32, (-1.5 + 0.5) * 32, (-2 + 14 + 0.5) * 32, (-1.5 + 7 + 0.5) * 32]
    rows[1] = [1, (W - 3 + 0.5) * 32, (H - 2 + 0.5) * 32, (W - 3 + 7 + 0.5) * 32, (H - 2 + 7 + 0.5) * 32]
    rows[2][0], rows[3][0] = -1, N
    rois = torch.tensor(rows, dtype=torch.float32)
    ys, xs, b = sample_coords(rois, EXACT_SIZE, EXACT_SCALE, EXACT_SR, True)
    inside = (b >= 0) & (b < N)
    assert (ys[inside] < -1).any() and ((ys[inside] >= -1) & (ys[inside] <= 0)).any() and (xs[inside] > W).any()
    assert (~inside).sum() == 2 and (b < 0).any() and (b >= N).any()
    assert torch.equal(ys * 16, (ys * 16).round()) and torch.equal(xs * 16, (xs * 16).round())
    x = torch.randint(-8, 9, (N, C, H, W), generator=g).float() / 8
    grad_out = torch.randint(-4, 5, (K, C, EXACT_SIZE, EXACT_SIZE), generator=g).float() / 4
    mag = reference_backward(x.shape, rois, grad_out.abs(), EXACT_SIZE, EXACT_SCALE, EXACT_SR, True)
    assert mag.max().item() < 2 ** 12, "the term magnitudes of one element sum to 2^12 or more: partial sums of 2^-12 steps may not be fp32 numbers"
    assert torch.equal(mag * 4096, (mag * 4096).round())
    return x, rois, grad_out
