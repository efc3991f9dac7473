"""ResNet-50 body with torchvision's parameter names, written here because torchvision is not
part of this stack.  The reference instantiates ``torchvision.models.resnet50(
replace_stride_with_dilation=[False, False, dilation], norm_layer=FrozenBatchNorm2d)``
(/root/reference/models/backbone_scratch.py:156-159); this module reproduces that architecture
(v1.5 bottleneck: stride on the 3x3 conv; a dilated stage keeps dilation 1 in its first block and
uses the new dilation afterwards) so reference checkpoints load key-for-key:
``conv1, bn1, layer{1..4}.{i}.conv{1,2,3}, .bn{1,2,3}, .downsample.{0,1}``.
torchvision itself is third-party and absent from /root/reference: PARITY UNPINNED for the
architecture; numerics are plain conv2d and pinned by torch.
"""
import torch
from torch import nn

import os

from dfx import ops as _ops

from .fused import derived_key, needs_grad

_PAIR_SHORTCUT = os.environ.get("DFX_PAIR_SHORTCUT", "1") == "1"      # A/B switch of the fused conv3 + shortcut product
_CONV_CHAIN = os.environ.get("DFX_CONV_CHAIN", "1") == "1"            # A/B switch of conv3 + the next block's conv1 in one launch
# widest conv1 the chain takes: 256 output channels (layer2[3] -> layer3[0]) leave the fused kernel one workgroup per CU and
# measured 4 % slower than the two launches at 32 frames, every narrower producer 7-25 % faster (profiles/r10_conv1x1_chain.txt)
_CONV_CHAIN_MAX_C1 = int(os.environ.get("DFX_CONV_CHAIN_MAX_C1", "128"))


def _fold(conv, bn):
    """Conv weight with the frozen-BN scale folded in, and the remaining per-channel shift."""
    scale, shift = bn.scale_shift()
    return (conv.weight.detach() * scale.reshape(-1, 1, 1, 1)).contiguous(), shift.detach().contiguous()


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride, dilation, downsample, norm_layer):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = norm_layer(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def _folded_params(self):
        mods = [self.conv1, self.bn1, self.conv2, self.bn2, self.conv3, self.bn3]
        if self.downsample is not None:
            mods += [self.downsample[0], self.downsample[1]]
        key = derived_key(*mods)
        if self.__dict__.get("_folded") is None or self._folded[0] != key:
            c2 = self.conv2
            scale2, shift2 = self.bn2.scale_shift()
            # conv2 on the hand-written kernels (Winograd F(2x2,3x3) for stride 1 incl. the dilated stage,
            # implicit GEMM for stride 2): folded-BN scale in the weights, shift + ReLU in the epilogue
            plan2 = _ops.ConvPlan(c2.weight, shift2.detach(), c2.stride, c2.padding, c2.dilation, "relu",
                                  scale=scale2.detach(), groups=c2.groups, padding_mode=c2.padding_mode)
            f = [_fold(self.conv1, self.bn1), plan2, _fold(self.conv3, self.bn3)]
            f.append(_fold(self.downsample[0], self.downsample[1]) if self.downsample is not None else None)
            # a stride-1 projection shortcut (layer1[0]; layer4[0] of the dilated DC5 stage) joins conv3 in ONE product over
            # the concatenated input channels: W = [W3 | Wd], bias = shift3 + shiftd (dfx.ops.conv1x1_pair)
            pair = None
            if self.downsample is not None and self.downsample[0].stride[0] == 1 and _PAIR_SHORTCUT:
                (w3, b3), (wd, bd) = f[2], f[3]
                if w3.shape[1] % 16 == 0 and wd.shape[1] % 16 == 0:
                    pair = (torch.cat([w3.flatten(1), wd.flatten(1)], 1).contiguous(), (b3 + bd).contiguous())
            f.append(pair)
            self._folded = (key, f)
        return self._folded[1]

    def chain_conv1(self):
        """Folded (weight, bias) of conv1 for the block in front to compute with its own conv3 (dfx.ops.conv1x1_chain), or
        None: torchvision puts a stage's stride on conv2, so conv1 is a stride-1 1x1 product over the map it is handed."""
        c = self.conv1
        if c.kernel_size != (1, 1) or c.stride != (1, 1) or c.padding != (0, 0) or c.groups != 1:
            return None
        return self._folded_params()[0]

    def forward_fused(self, x, z=None, nxt=None):
        """Inference on the GPU: frozen BN folded into the convolutions.  The 3x3 convolutions run on the
        hand-written Winograd / implicit-GEMM kernels (dfx.ops.ConvPlan, csrc/conv_wino.hip,
        csrc/conv_igemm.hip), the 1x1 convolutions on the hand-written MFMA GEMM (dfx.ops.conv1x1), each
        with bias / residual / ReLU in its epilogue.  No CPU route.

        z: this block's conv1 output where the block in front has already computed it.  nxt: the folded conv1 of the block
        that follows (chain_conv1()); the result is then (y, z_next) with z_next that block's conv1 output from the same
        launch as conv3 (csrc/conv1x1_chain.hip), or None where the fused kernel does not cover the shape."""
        (w1, b1), plan2, (w3, b3), down, pair = self._folded_params()
        out = z if z is not None else self._conv1x1(0, x, w1, b1, relu=True)
        out = plan2(out)
        hw = out.shape[2] * out.shape[3]
        chain = nxt is not None and hw % 4 == 0 and nxt[0].shape[0] <= _CONV_CHAIN_MAX_C1
        if pair is not None and hw % 4 == 0 and out.shape[2:] == x.shape[2:]:
            if chain and _ops.conv1x1_chain_supported(pair[0].shape[0], out.shape[1], x.shape[1], nxt[0].shape[0], hw):
                return _ops.conv1x1_chain(out, pair[0], pair[1], nxt[0], nxt[1], x2=x.contiguous())
            y = _ops.conv1x1_pair(out, x.contiguous(), pair[0], pair[1], relu=True)
            return y if nxt is None else (y, None)
        if down is not None:
            x = self._conv1x1(1, x, down[0], down[1], relu=False, stride=self.downsample[0].stride[0])
        if chain and _ops.conv1x1_chain_supported(w3.shape[0], out.shape[1], 0, nxt[0].shape[0], hw):
            return _ops.conv1x1_chain(out, w3, b3, nxt[0], nxt[1], residual=x)
        y = self._conv1x1(2, out, w3, b3, relu=True, residual=x)
        return y if nxt is None else (y, None)

    def _conv1x1(self, slot, x, w, b, relu, residual=None, stride=1):
        """1x1 convolution + bias (+ residual) (+ ReLU): the MFMA GEMM over [Ci] x [H*W] when its 16-byte
        operand rows allow (H*W a multiple of 4: every map of an 800x1333 frame), else the implicit-GEMM
        convolution (scalar gathers, any geometry) followed by the fused bias / residual / ReLU pass."""
        ho, wo = (x.shape[2] + stride - 1) // stride, (x.shape[3] + stride - 1) // stride
        if (ho * wo) % 4 == 0 and stride == 1:
            return _ops.conv1x1(x, w, b, residual=residual, relu=relu, stride=stride)
        # strided shortcut (the implicit GEMM gathers every other pixel itself: no subsampled copy of the map) and
        # maps whose rows are not 16-byte aligned
        # keyed on the version key of the parameters the folded tensors were made from (the folded temporaries' own
        # addresses / versions say nothing: the allocator hands an address out again after a refold)
        key = self._folded[0]
        plans = self.__dict__.setdefault("_plans1x1", {})
        fused = residual is None
        if slot not in plans or plans[slot][0] != key:
            plans[slot] = (key, _ops.ConvPlan(w.reshape(w.shape[0], -1, 1, 1), b if fused else None, stride, 0, 1,
                                              "relu" if (fused and relu) else None))
        y = plans[slot][1](x)
        return y if fused else _ops.bias_act_(y, b, residual=residual, relu=relu)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        skip = x if self.downsample is None else self.downsample(x)
        return self.relu(out + skip)


class ResNet50(nn.Module):
    def __init__(self, norm_layer, replace_stride_with_dilation=(False, False, False)):
        super().__init__()
        self.inplanes, self.dilation = 64, 1
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._stage(64, 3, 1, False, norm_layer)
        self.layer2 = self._stage(128, 4, 2, replace_stride_with_dilation[0], norm_layer)
        self.layer3 = self._stage(256, 6, 2, replace_stride_with_dilation[1], norm_layer)
        self.layer4 = self._stage(512, 3, 2, replace_stride_with_dilation[2], norm_layer)
        # torchvision's resnet50 also owns the ImageNet classifier; the detectors never call it, but a reference checkpoint
        # carries `backbone.0.body.fc.{weight,bias}` and a strict load (benchmark.py:58) needs somewhere to put them
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, 1000)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _stage(self, planes, blocks, stride, dilate, norm_layer):
        first_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False),
                                       norm_layer(planes * 4))
        layers = [Bottleneck(self.inplanes, planes, stride, first_dilation, downsample, norm_layer)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, 1, self.dilation, None, norm_layer))
        return nn.Sequential(*layers)

    def stem(self, x, fused=False):
        if not fused:
            return self.maxpool(self.relu(self.bn1(self.conv1(x))))
        key = derived_key(self.conv1, self.bn1)
        if self.__dict__.get("_stem_folded") is None or self._stem_folded[0] != key:
            scale, shift = self.bn1.scale_shift()
            self._stem_folded = (key, (_ops.ConvPlan(self.conv1.weight, None, 2, 3, 1, None, scale=scale.detach()),
                                       shift.detach().contiguous()))
        plan, b = self._stem_folded[1]
        return _ops.bias_relu_maxpool(plan(x), b)

    def run_stage(self, stage, x, fused=False):
        if not fused:
            return stage(x)
        # conv3 of a layer1 / layer2 block also produces the conv1 of the block behind it - the next block of the stage or
        # the first one of the next stage - in the same launch where that measured faster (_CONV_CHAIN_MAX_C1): these producers are
        # HBM-bound on writing their 256- / 512-channel map, which the standalone conv1 would read back in full.  layer3 /
        # layer4 producers are MFMA-bound and stay as they are.  Between two stages the pair (map, its conv1) waits in
        # _chain_carry; it is used only for the very tensor it was computed from.
        carry, self._chain_carry = self.__dict__.get("_chain_carry"), None
        z = carry[1] if carry is not None and carry[0] is x else None
        follower = {id(self.layer1): self.layer2, id(self.layer2): self.layer3}.get(id(stage)) if _CONV_CHAIN else None
        # a stage that trains runs op by op (models.backbone_scratch.FusionBackboneBase.forward): its first conv1 is not
        # computed here from detached folded weights, and no carry is left waiting for it (this stage's output carries no
        # gradient, so the follower's own parameters decide)
        across = follower is not None and not needs_grad(follower)
        blocks = list(stage)
        for i, block in enumerate(blocks):
            succ = None
            if follower is not None:
                succ = blocks[i + 1] if i + 1 < len(blocks) else (follower[0] if across else None)
            nxt = succ.chain_conv1() if succ is not None else None
            if nxt is None:
                x, z = block.forward_fused(x, z), None
            else:
                x, z = block.forward_fused(x, z, nxt)
        if z is not None:
            self._chain_carry = (x, z)
        return x

    def forward(self, x):
        x = self.stem(x)
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))
