"""TEST INFRASTRUCTURE: a tiny stereo network with the class and attribute names harness.fuse looks for (BasicConv, Conv2x,
SGABlock, CostAggregation, DispAgg, GetCostVolume; conv_start / conv1a / deconv1a / sga1 / sga11 / sga2 / disp1 / cv), so that
use_mixed_precision can be run end to end on the device where the reference's model files are not available.  BasicConv,
SGABlock and DispAgg are those of tests/standin_net.py (which has the training-capable network); here the rebound forwards
are the thing under test, at 4 channels, one level and inference only."""
import torch
from torch import nn

from ganet_amd.modules.GANet import GetCostVolume
from standin_net import BasicConv, DispAgg, SGABlock      # noqa: F401  (the blocks are tests/standin_net.py's)

C = 4            # channels of the cost-aggregation volumes


class Conv2x(nn.Module):
    def __init__(self, c, relu=True):
        super().__init__()
        self.conv1 = BasicConv(c, c, True, kernel_size=3, padding=1)
        self.conv2 = BasicConv(2 * c, c, True, relu=relu, kernel_size=3, padding=1)

    def forward(self, x, rem):
        return self.conv2(torch.cat((self.conv1(x), rem), 1))


class CostAggregation(nn.Module):
    def __init__(self, maxdisp):
        super().__init__()
        self.conv_start = BasicConv(16, C, True, relu=False, kernel_size=3, padding=1)
        self.conv1a = BasicConv(C, C, True, kernel_size=3, padding=1)
        self.deconv1a = Conv2x(C, relu=False)
        self.sga1, self.sga11, self.sga2 = SGABlock(C, True), SGABlock(C, True), SGABlock(C, True)
        self.disp1 = DispAgg(maxdisp, C)

    def forward(self, x, g):
        x = self.sga1(self.conv_start(x), g["sg1"])
        rem0 = x
        x = self.sga11(self.conv1a(x), g["sg11"])
        x = self.sga2(self.deconv1a(x, rem0), g["sg2"])
        return self.disp1(x, g["lg1"], g["lg2"])


class GANet(nn.Module):
    """left, right [N, 3, 3h, 3w] -> disparity [N, 3h, 3w].  The guidance branch has the reference's shape at the top level: a
    plain convolution on the low-resolution features, a bilinear up-sampling (which torch.autocast runs in fp32), a
    Sequential(BatchNorm2d, ReLU), a concatenation with a full-resolution feature map and a BasicConv behind it."""

    def __init__(self, maxdisp=12):
        super().__init__()
        self.feature = BasicConv(3, 8, kernel_size=3, stride=3)
        self.guide_small = BasicConv(3, 8, kernel_size=3, stride=3)
        self.guide_full = BasicConv(3, 8, kernel_size=3, padding=1)
        self.weight_sg = nn.ModuleDict({k: nn.Conv2d(8, 20 * C, 3, 1, 1, bias=False) for k in ("sg1", "sg11", "sg2")})
        self.weight_lg = nn.ModuleDict({k: nn.Conv2d(8, 75, 3, 1, 1, bias=False) for k in ("lg1", "lg2")})
        self.conv_refine = nn.Conv2d(8, 16, (3, 3), (1, 1), (1, 1), bias=False)
        self.bn_relu = nn.Sequential(nn.BatchNorm2d(16), nn.ReLU(inplace=True))
        self.guide_mix = BasicConv(24, 8, kernel_size=3, padding=1)
        self.cost_agg = CostAggregation(maxdisp)
        self.cv = GetCostVolume(int(maxdisp / 3))
        gen = torch.Generator().manual_seed(11)
        for m in self.modules():                  # statistics that make the fold more than the identity
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                with torch.no_grad():
                    m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                    m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                    m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                    m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.1)

    def forward(self, left, right):
        fl = self.feature(left)
        x1 = torch.nn.functional.interpolate(self.conv_refine(fl), [3 * fl.shape[2], 3 * fl.shape[3]], mode="bilinear", align_corners=False)
        gs, gf = self.guide_small(left), self.guide_mix(torch.cat((self.guide_full(left), self.bn_relu(x1)), 1))
        g = {k: conv(gs) for k, conv in self.weight_sg.items()}
        g.update({k: conv(gf) for k, conv in self.weight_lg.items()})
        cost = self.cv(fl, self.feature(right))
        return self.cost_agg(cost, g)
