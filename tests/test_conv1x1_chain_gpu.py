"""GPU: a bottleneck's conv3 and the next block's conv1 as one launch (csrc/conv1x1_chain.hip, dfx.ops.conv1x1_chain)
against float64, against the two separate launches it replaces, and through models/resnet.py.

Bounds (fp32 MFMA is an exact-fp32 k-ordered fma chain: tests/test_gemm_gpu.py): Y within 4e-6 * sqrt(K) of the fp64
product (K = K1 + K2 in the two-segment form), Z within 4e-6 * sqrt(Co) of fp64 computed from the kernel's own fp32 Y.
The first product runs gemm_f32_kernel's k order and epilogue order and a wave sums Z over all of Co in that same order,
so both outputs are also asserted bit-equal to ops.conv1x1 / ops.conv1x1_pair followed by ops.conv1x1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (Co, K1, K2, C1, H, W, N, bias, relu_z)
CASES = [
    (256, 64, 0, 64, 6, 10, 2, True, True),        # plain form with a residual (layer1[1,2])
    (512, 128, 0, 128, 5, 12, 2, True, True),      # 16 channel tiles, the K = 128 panel (layer2[1..3])
    (256, 64, 64, 64, 6, 10, 2, True, True),       # two-segment form, no residual (layer1[0])
    (256, 64, 0, 128, 7, 12, 2, True, True),       # HW = 84: no multiple of 32, the last wave's tile is partly empty (layer2[0])
    (512, 128, 0, 256, 5, 12, 1, True, True),      # C1 = 256: one workgroup per CU (layer3[0])
    (64, 64, 0, 256, 6, 10, 1, True, False),
    (64, 32, 0, 32, 8, 16, 2, True, True),         # HW = 128: exactly one workgroup tile
    (64, 32, 0, 32, 11, 12, 2, True, False),       # HW = 132: one pixel quad into the second tile
    (32, 32, 0, 32, 6, 10, 1, True, True),         # minimum channels: every panel half empty
    (96, 96, 0, 96, 7, 12, 1, True, True),         # channel counts between two instantiations (zero-filled panels)
    (96, 48, 48, 96, 6, 10, 2, False, False),
    (256, 64, 0, 64, 6, 10, 3, False, True),       # three frames, no bias
    (256, 64, 0, 64, 6, 10, 3, True, False),       # no ReLU on Z
    (128, 16, 16, 64, 9, 12, 3, False, True),
]


def _inputs(Co, K1, K2, C1, H, W, N):
    g = torch.Generator().manual_seed(Co + 3 * K1 + 5 * K2 + 7 * C1 + H * W)
    x = torch.randn(N, K1, H, W, generator=g).cuda()
    x2 = torch.randn(N, K2, H, W, generator=g).cuda() if K2 else None
    w3 = (torch.randn(Co, K1 + K2, generator=g) / (K1 + K2) ** 0.5).cuda()
    b3 = torch.randn(Co, generator=g).cuda()
    res = None if K2 else torch.randn(N, Co, H, W, generator=g).cuda()
    w1 = (torch.randn(C1, Co, generator=g) / Co ** 0.5).cuda()
    b1 = torch.randn(C1, generator=g).cuda()
    return x, x2, w3, b3, res, w1, b1


def _check_fp64(y, z, x, x2, w3, b3, res, w1, b1, relu_z):
    K, Co = w3.shape[1], w3.shape[0]
    xin = x if x2 is None else torch.cat([x, x2], 1)
    want = torch.einsum("ok,nkhw->nohw", w3.double(), xin.double())
    if b3 is not None:
        want = want + b3.double().view(1, -1, 1, 1)
    if res is not None:
        want = want + res.double()
    want = want.relu()
    ey = (y.double() - want).abs().max().item()
    wz = torch.einsum("ok,nkhw->nohw", w1.double(), y.double())
    if b1 is not None:
        wz = wz + b1.double().view(1, -1, 1, 1)
    wz = wz.relu() if relu_z else wz
    ez = (z.double() - wz).abs().max().item()
    print(f"chain Co={Co} K={K} C1={w1.shape[0]} HW={x.shape[2] * x.shape[3]}: Y err {ey:.3e} (bound {4e-6 * K ** 0.5:.3e}), "
          f"Z err {ez:.3e} (bound {4e-6 * Co ** 0.5:.3e})")
    assert ey < 4e-6 * K ** 0.5
    assert ez < 4e-6 * Co ** 0.5


@pytest.mark.parametrize("Co,K1,K2,C1,H,W,N,bias,relu_z", CASES)
def test_conv1x1_chain_matches_fp64_and_the_two_launches(Co, K1, K2, C1, H, W, N, bias, relu_z):
    from dfx import ops
    assert ops.conv1x1_chain_supported(Co, K1, K2, C1, H * W)
    x, x2, w3, b3, res, w1, b1 = _inputs(Co, K1, K2, C1, H, W, N)
    if not bias:
        b3 = b1 = None
    y, z = ops.conv1x1_chain(x, w3, b3, w1, b1, residual=res, x2=x2, relu_z=relu_z)
    assert y.shape == (N, Co, H, W) and z.shape == (N, C1, H, W)
    _check_fp64(y, z, x, x2, w3, b3, res, w1, b1, relu_z)
    # the first product runs the existing K loop order and register epilogue order: Y is bit-equal to today's launch, and
    # so is Z (one wave sums all of Co in ascending k pairs, the standalone kernel's order)
    y2 = ops.conv1x1(x, w3, b3, residual=res, relu=True) if x2 is None else ops.conv1x1_pair(x, x2, w3, b3, relu=True)
    assert torch.equal(y, y2)
    assert torch.equal(z, ops.conv1x1(y2, w1, b1, relu=relu_z))


def test_conv1x1_chain_leaves_the_neighbouring_memory_alone():
    """Ragged pixel tail and channel panels: nothing is written outside Y and Z (buffers with guard bands)."""
    from dfx import _lib, ops
    Co, K, C1, H, W, N = 96, 32, 32, 7, 12, 2
    x, _, w3, b3, res, w1, b1 = _inputs(Co, K, 0, C1, H, W, N)
    HW, guard = H * W, 512
    ybuf = torch.full((N * Co * HW + 2 * guard,), 7.0, device="cuda")
    zbuf = torch.full((N * C1 * HW + 2 * guard,), 7.0, device="cuda")
    rc = _lib.load().dfx_conv1x1_chain_f32(w3.data_ptr(), x.data_ptr(), K * HW, K, 0, 0, 0, b3.data_ptr(), res.data_ptr(), Co * HW,
                                           ybuf.data_ptr() + guard * 4, Co * HW, w1.data_ptr(), b1.data_ptr(),
                                           zbuf.data_ptr() + guard * 4, C1 * HW, Co, C1, HW, N, 1,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    y, z = ops.conv1x1_chain(x, w3, b3, w1, b1, residual=res)
    for buf, t in ((ybuf, y), (zbuf, z)):
        assert torch.equal(buf[guard:-guard].view_as(t), t)
        assert (buf[:guard] == 7.0).all() and (buf[-guard:] == 7.0).all()


@pytest.mark.parametrize("Co,K1,K2,C1", [(40, 24, 0, 20), (64, 160, 0, 64), (64, 64, 0, 288), (64, 32, 32, 48)])
def test_unsupported_shapes_take_the_two_launches(Co, K1, K2, C1):
    """Outside the fused kernel's shapes the entry point returns its error code without a launch and the wrapper runs the
    two separate launches: same results."""
    from dfx import _lib, ops
    H, W, N = 6, 10, 2
    assert not ops.conv1x1_chain_supported(Co, K1, K2, C1, H * W)
    x, x2, w3, b3, res, w1, b1 = _inputs(Co, K1, K2, C1, H, W, N)
    one = 16
    rc = _lib.load().dfx_conv1x1_chain_f32(one, one, K1 * H * W, K1, one if K2 else 0, K2 * H * W, K2, 0, 0, 0, one, Co * H * W,
                                           one, 0, one, C1 * H * W, Co, C1, H * W, N, 1, None)
    assert rc == -1 and b"conv1x1_chain" in _lib.load().dfx_last_error()
    y, z = ops.conv1x1_chain(x, w3, b3, w1, b1, residual=res, x2=x2)
    y2 = ops.conv1x1(x, w3, b3, residual=res, relu=True) if x2 is None else ops.conv1x1_pair(x, x2, w3, b3, relu=True)
    assert torch.equal(y, y2) and torch.equal(z, ops.conv1x1(y2, w1, b1, relu=True))
    _check_fp64(y, z, x, x2, w3, b3, res, w1, b1, True)


def test_resnet_layers_agree_with_the_chain_on_and_off(monkeypatch):
    """models/resnet.py at 2 frames of 64x96: every layer output with conv3 + next conv1 chained (all seven producers of
    layer1 and layer2, the last one feeding layer3[0]; and the shipped routing, which leaves that 256-channel conv1 to its
    own launch) against the separate launches, within the bound of test_fused_backbone_matches_reference_formulation
    (1e-4 of the map's scale)."""
    import models.resnet as resnet
    from dfx import ops
    from models.backbone_scratch import build_backbone_fromscratch
    from models.config import single_args
    from models.fused import enable_fused_inference
    from tests._param_fill import fill_params_by_name
    args = single_args("Baseline")
    args.depth_type = "Baseline_rgb"
    bb = fill_params_by_name(build_backbone_fromscratch(args), seed=3).cuda().eval()
    assert enable_fused_inference(bb) >= 1
    body = bb[0].body
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    calls = []
    chain = ops.conv1x1_chain
    monkeypatch.setattr(ops, "conv1x1_chain", lambda *a, **k: (calls.append(a[0].shape), chain(*a, **k))[1])

    def layers(on, max_c1=256):
        monkeypatch.setattr(resnet, "_CONV_CHAIN", on)
        monkeypatch.setattr(resnet, "_CONV_CHAIN_MAX_C1", max_c1)
        del calls[:]
        outs = []
        with torch.no_grad():
            t = body.stem(x, True)
            for stage in (body.layer1, body.layer2, body.layer3, body.layer4):
                t = body.run_stage(stage, t, True)
                outs.append(t)
        return outs, len(calls)

    off, n_off = layers(False)
    on, n_on = layers(True)
    routed, n_routed = layers(True, 128)
    assert n_off == 0 and n_on == 7 and n_routed == 6
    for a, b in list(zip(off, on)) + list(zip(off, routed)):
        scale = a.abs().max().item()
        err = (a - b).abs().max().item()
        print(f"layer {tuple(a.shape)}: chain on vs off max abs diff {err:.3e} (scale {scale:.3e})")
        assert a.shape == b.shape and err < 1e-4 * max(scale, 1.0)
