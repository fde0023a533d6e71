"""TEST INFRASTRUCTURE: a small stereo network that stands for the reference's GANet_deep wherever its model files are not
available -- the device machine above all.  It is written from INTEGRATION.md (the call-site edits), SURVEY.md Appendix B (the
op census) and the docstring of harness/fuse.py (which lines each rebinder replaces); nothing of the reference is in it.

It carries the class and attribute names harness.fuse dispatches on (BasicConv: conv / bn / relu / use_bn; Conv2x: conv1 /
conv2; SGABlock: refine / bn_relu / conv_refine / bn; Disp and DispAgg: maxdisp / conv32x1; CostAggregation: the producers of
fuse._SGA_PRODUCER in front of sga1 / sga11 / sga2 / sga3; GANet: cost_agg / cv), and -- unlike the fragments inside
tests/test_gpu_bn.py, test_gpu_disp_tail.py and test_gpu_disp_conv.py -- every block has a STOCK forward on the drop-in modules of
ganet_amd.modules.GANet (SGA, LGA2, GetCostVolume, DisparityRegression), so that one model runs un-rebound, under every
rebinder of harness.fuse, in training and in inference, and on the CPU through oracle.cpu_ops.route_cpu_through_oracle.
tests/test_model_calls_cpu.py ties SGABlock, Disp and DispAgg to the reference's classes (same state_dict, same bits, same
rebinder counts) where the reference exists.

The shape of GANet_deep in miniature: features at a third of the image, a cost volume of maxdisp / 3 + 1 planes, an hourglass
of 3-D convolutions over two levels (a third and a sixth) with four SGABlocks -- three with `refine`, the last without, on its
own `bn` -- two Disp tails (training only) and one DispAgg.  C = 8 aggregation channels; at maxdisp = 48 and a 48 x 96 crop the
SGA volumes are [1,8,17,16,32] and [1,8,9,8,16], LGA runs at [1,49,48,96] with radius 2, DispConv on [1,8,17,16,32]."""
import torch
import torch.nn.functional as F
from torch import nn

from ganet_amd.modules.GANet import LGA2, SGA, DisparityRegression, GetCostVolume

C = 8            # channels of the cost-aggregation volumes


class BasicConv(nn.Module):
    """convolution (2-D | 3-D, plain | transposed) -> BatchNorm -> ReLU, the last two optional"""

    def __init__(self, cin, cout, is_3d=False, relu=True, deconv=False, bn=True, **kw):
        super().__init__()
        self.relu, self.use_bn = relu, bn
        if is_3d:
            self.conv = (nn.ConvTranspose3d if deconv else nn.Conv3d)(cin, cout, bias=False, **kw)
            self.bn = nn.BatchNorm3d(cout)
        else:
            self.conv = (nn.ConvTranspose2d if deconv else nn.Conv2d)(cin, cout, bias=False, **kw)
            self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        x = self.conv(x)
        if self.use_bn:
            x = self.bn(x)
        return F.relu(x, inplace=True) if self.relu else x


class Conv2x(nn.Module):
    """to the other level of the hourglass (stride 2: down, or transposed: up), the skip connection concatenated, one more
    convolution: [N,cin,..] and rem [N,cout,..] -> [N,cout,..] at rem's size"""

    def __init__(self, cin, cout, deconv=False, relu=True):
        super().__init__()
        if deconv:
            self.conv1 = BasicConv(cin, cout, True, deconv=True, kernel_size=(3, 4, 4), stride=2, padding=1)
        else:
            self.conv1 = BasicConv(cin, cout, True, kernel_size=3, stride=2, padding=1)
        self.conv2 = BasicConv(2 * cout, cout, True, relu=relu, kernel_size=3, stride=1, padding=1)

    def forward(self, x, rem):
        x = self.conv1(x)
        assert x.size() == rem.size(), (x.size(), rem.size())
        return self.conv2(torch.cat((x, rem), 1))


class SGABlock(nn.Module):
    """x [N,C,D,H,W], g [N,20C,H,W] -> relu(conv_refine(bn_relu(SGA(x, k1..k4))) + x), k = the four L1-normalised [N,C,5,H,W]
    groups of g; refine=False: relu(bn(SGA(..)) + x)"""

    def __init__(self, channels=32, refine=False):
        super().__init__()
        self.refine = refine
        if refine:
            self.bn_relu = nn.Sequential(nn.BatchNorm3d(channels), nn.ReLU(inplace=True))
            self.conv_refine = BasicConv(channels, channels, True, relu=False, kernel_size=3, padding=1)
        else:
            self.bn = nn.BatchNorm3d(channels)
        self.SGA = SGA()
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x, g):
        rem = x
        N, _, H, W = g.shape
        ks = [F.normalize(k.view(N, x.size(1), -1, H, W), p=1, dim=2) for k in torch.split(g, x.size(1) * 5, 1)]
        x = self.SGA(x, *ks)
        if self.refine:
            x = self.conv_refine(self.bn_relu(x))
        else:
            x = self.bn(x)
        x += rem
        return self.relu(x)


class Disp(nn.Module):
    """x [N,channels,D,H,W] -> the disparity map [N,3H,3W]: conv32x1, trilinear up-sampling to maxdisp + 1 planes at three
    times the size, Softmin over the planes, regression"""

    def __init__(self, maxdisp=192, channels=32):
        super().__init__()
        self.maxdisp = maxdisp
        self.softmin = nn.Softmin(dim=1)
        self.regression = DisparityRegression(maxdisp=self.maxdisp)
        self.conv32x1 = nn.Conv3d(channels, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False)

    def forward(self, x):
        x = F.interpolate(self.conv32x1(x), [self.maxdisp + 1, x.size()[3] * 3, x.size()[4] * 3], mode="trilinear", align_corners=False)
        x = torch.squeeze(x, 1)
        return self.regression(self.softmin(x))


class DispAgg(nn.Module):
    """the last tail: the same up-sampling, then LGA2 on filters lg1, Softmin, LGA2 on lg2 (both [N,75,3H,3W], L1-normalised
    over the taps), L1-normalisation along the disparity axis, regression"""

    def __init__(self, maxdisp=192, channels=32):
        super().__init__()
        self.maxdisp = maxdisp
        self.LGA2 = LGA2(radius=2)
        self.softmin = nn.Softmin(dim=1)
        self.regression = DisparityRegression(maxdisp=self.maxdisp)
        self.conv32x1 = nn.Conv3d(channels, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False)

    def lga(self, x, g):
        return self.LGA2(x, F.normalize(g, p=1, dim=1))

    def forward(self, x, lg1, lg2):
        x = F.interpolate(self.conv32x1(x), [self.maxdisp + 1, x.size()[3] * 3, x.size()[4] * 3], mode="trilinear", align_corners=False)
        x = torch.squeeze(x, 1)
        assert lg1.size() == lg2.size()
        x = self.lga(x, lg1)
        x = self.softmin(x)
        x = self.lga(x, lg2)
        x = F.normalize(x, p=1, dim=1)
        return self.regression(x)


class CostAggregation(nn.Module):
    """cost [N,2F,D,h,w] and the guidance dict -> three disparity maps in training mode (disp0 behind sga1, disp1 behind sga2,
    disp2 = DispAgg behind sga3), the last one alone in eval mode"""

    def __init__(self, maxdisp=192, channels=C, features=8):
        super().__init__()
        self.maxdisp = maxdisp
        c = channels
        self.conv_start = BasicConv(2 * features, c, True, relu=False, kernel_size=3, padding=1)
        self.conv1a = BasicConv(c, c, True, kernel_size=3, stride=2, padding=1)
        self.deconv1a = Conv2x(c, c, deconv=True, relu=False)
        self.conv1b = Conv2x(c, c)
        self.deconv1b = Conv2x(c, c, deconv=True, relu=False)
        self.sga1 = SGABlock(c, refine=True)
        self.sga11 = SGABlock(c, refine=True)
        self.sga2 = SGABlock(c, refine=True)
        self.sga3 = SGABlock(c, refine=False)
        self.disp0 = Disp(maxdisp, c)
        self.disp1 = Disp(maxdisp, c)
        self.disp2 = DispAgg(maxdisp, c)

    def forward(self, x, g):
        x = self.sga1(self.conv_start(x), g["sg1"])
        rem0 = x
        disp0 = self.disp0(x) if self.training else None
        x = self.sga11(self.conv1a(x), g["sg11"])
        rem1 = x
        x = self.sga2(self.deconv1a(x, rem0), g["sg2"])
        rem0 = x
        disp1 = self.disp1(x) if self.training else None
        x = self.conv1b(x, rem1)
        x = self.sga3(self.deconv1b(x, rem0), g["sg3"])
        disp2 = self.disp2(x, g["lg1"], g["lg2"])
        return (disp0, disp1, disp2) if self.training else disp2


def seed_batchnorms(model, seed=11):
    """running statistics and affine parameters from a fixed seed: the eval-mode fold is more than the identity"""
    gen = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.1)


class GANet(nn.Module):
    """left, right [N,3,3h,3w] (h even) -> what CostAggregation returns.  Features and the semi-global guidance at a third of
    the image (sg11 at a sixth), the local filters at full size."""

    FEATURES = 8

    def __init__(self, maxdisp=48, channels=C):
        super().__init__()
        self.maxdisp = maxdisp
        f = self.FEATURES
        self.feature = BasicConv(3, f, kernel_size=3, stride=3)
        self.guide_small = BasicConv(3, f, kernel_size=3, stride=3)
        self.guide_down = BasicConv(f, f, kernel_size=3, stride=2, padding=1)
        self.guide_full = BasicConv(3, f, kernel_size=3, padding=1)
        self.weight_sg = nn.ModuleDict({k: nn.Conv2d(f, 20 * channels, (3, 3), (1, 1), (1, 1), bias=False) for k in ("sg1", "sg2", "sg3", "sg11")})
        self.weight_lg = nn.ModuleDict({k: nn.Conv2d(f, 75, (3, 3), (1, 1), (1, 1), bias=False) for k in ("lg1", "lg2")})
        self.cost_agg = CostAggregation(maxdisp, channels, f)
        self.cv = GetCostVolume(int(maxdisp / 3))
        seed_batchnorms(self)

    def forward(self, left, right):
        gs = self.guide_small(left)
        gd, gf = self.guide_down(gs), self.guide_full(left)
        g = {k: conv(gd if k == "sg11" else gs) for k, conv in self.weight_sg.items()}
        g.update({k: conv(gf) for k, conv in self.weight_lg.items()})
        cost = self.cv(self.feature(left), self.feature(right))
        return self.cost_agg(cost, g)


def build(maxdisp=48, device="cpu", seed=0):
    """the network with seeded weights, on `device`"""
    torch.manual_seed(seed)
    return GANet(maxdisp).to(device)
