"""ResNet-50 for the flagship images/sec benchmark (BASELINE.json
configs 2-3), written from scratch.

MI355X mapping: convolutions go through MIOpen (channels_last + bf16
autocast picks the implicit-GEMM MFMA paths) under the committed tuning,
except the forward of the stride-1 1x1 convolutions with Cin <= 256
(conv1/bn1, conv3/bn3 and the first stage's down_conv/down_bn, called
through sparkdl.ops.functional.conv1x1_bn_act): in training mode it runs
the in-house conv1x1_stats kernel, which reads the input once and writes
the BatchNorm partial sums in its epilogue, so the BatchNorm that follows
skips its statistics pass over the convolution output. Which sites take
it is functional.CONV1X1_STATS_SITES, decided site by site by
scripts/probe_conv1x1_bn.py (profiles/probe_conv1x1_bn.log,
profiles/README.md "Round 7"); their dgrad and wgrad stay on MIOpen, and
SPARKDL_CONV1X1_STATS=0 restores the unfused route exactly. The all
in-house 1x1 package (sparkdl.ops.Conv1x1 with SPARKDL_CONV1X1=1/all)
stays opt-in. Every
BatchNorm/ReLU/residual-add runs through sparkdl.ops' fused bf16-NHWC
BatchNormAct2d kernels (SURVEY.md §2.2 N4/N5 — the conv-block epilogue
fusion); the stem's BatchNorm + ReLU + 3x3/2 max-pool is one kernel chain
(sparkdl.ops.functional.batch_norm_relu_maxpool: the full-resolution
activation, the pool indices and the full-resolution gradient are never
written; SPARKDL_FUSED_STEM=0 composes the two modules instead, with
bitwise the same results); the optimizer step is sparkdl.ops.FusedSGD (one launch for all
161 tensors); gradient all-reduce is the bucketed DistributedOptimizer.

Each block's output has two consumers, the next block's conv1 and its
residual branch (identity or down_conv). The blocks pass it on as a pair
(BatchNormAct2d ``fork=True``), so the backward of bn3 gets the two
gradients separately and adds them inside its reduction kernel, and the
masked sum that kernel writes doubles as the gradient of the residual
input: autograd's bf16 add pass and the separate residual-gradient store
are gone at the 15 such outputs. SPARKDL_FUSED_RESGRAD=0 restores the add,
with bitwise the same results. The stem's pooled output forks as a plain
tensor; autograd adds there.
"""

import torch
import torch.nn as nn

from sparkdl.ops import (BatchNormAct2d, Conv1x1, batch_norm_relu_maxpool,
                         conv1x1_bn_act)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, width, stride=1):
        super().__init__()
        cout = width * self.expansion
        self.conv1 = Conv1x1(cin, width)
        self.bn1 = BatchNormAct2d(width, relu=True)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1,
                               bias=False)
        self.bn2 = BatchNormAct2d(width, relu=True)
        self.conv3 = Conv1x1(width, cout)
        # bn3 fuses the residual add + final ReLU of the block
        self.bn3 = BatchNormAct2d(cout, relu=True)
        if stride != 1 or cin != cout:
            self.down_conv = Conv1x1(cin, cout, stride=stride)
            self.down_bn = BatchNormAct2d(cout, relu=False)
        else:
            self.down_conv = None

    def forward(self, x):
        """x: a tensor, or the pair a previous block returned. Returns
        the block's output as a pair (BatchNormAct2d, ``fork=True``):
        one member for the next block's conv1, the other for its
        identity or down_conv, so that bn3's backward receives the two
        gradients separately."""
        x, skip = x if isinstance(x, tuple) else (x, x)
        if self.down_conv is not None:
            idn = conv1x1_bn_act(skip, self.down_conv, self.down_bn)
        else:
            idn = skip
        out = conv1x1_bn_act(x, self.conv1, self.bn1)
        out = self.bn2(self.conv2(out))
        return conv1x1_bn_act(out, self.conv3, self.bn3, residual=idn,
                              fork=True)


class ResNet50(nn.Module):
    LAYERS = (3, 4, 6, 3)

    def __init__(self, num_classes=1000):
        super().__init__()
        self.stem_conv = nn.Conv2d(3, 64, 7, stride=2, padding=3,
                                   bias=False)
        self.stem_bn = BatchNormAct2d(64, relu=True)
        self.stem_pool = nn.MaxPool2d(3, stride=2, padding=1)
        cin = 64
        stages = []
        for i, blocks in enumerate(self.LAYERS):
            width = 64 * (2 ** i)
            stride = 1 if i == 0 else 2
            layer = []
            for b in range(blocks):
                layer.append(Bottleneck(cin, width, stride if b == 0 else 1))
                cin = width * Bottleneck.expansion
            stages.append(nn.Sequential(*layer))
        self.stages = nn.Sequential(*stages)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(2048, num_classes)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
        # zero-init the last BN in each block (standard ResNet recipe)
        for m in self.modules():
            if isinstance(m, Bottleneck):
                nn.init.zeros_(m.bn3.weight)

    def forward(self, x):
        # stem_bn + stem_pool as one kernel chain; the two modules stay
        # as the owners of the parameters, buffers and pool geometry
        bn = self.stem_bn
        x = batch_norm_relu_maxpool(
            self.stem_conv(x), bn.weight, bn.bias, bn.running_mean,
            bn.running_var, momentum=bn.momentum, eps=bn.eps,
            training=bn.training)
        # the last block's output has one consumer: with one member of
        # its pair unused, its bn3 runs the one-gradient backward
        x, _ = self.stages(x)
        x = self.pool(x).flatten(1)
        return self.fc(x)
