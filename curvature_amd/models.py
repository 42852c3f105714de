"""Plain ``torch.nn`` definitions of the benchmark networks (LeNet-5, ImageNet ResNet-18 / ResNet-50, DenseNet-121 / 161,
the grouped-convolution networks MobileNetV2 / ResNeXt-50 32x4d, and the upsampling networks DCGAN generator / U-Net
with ``ConvTranspose2d`` layers).

torchvision is not available on the target image, and the estimators select layers by class NAME
(``Conv2d`` / ``Linear``; curvature/curvatures.py:121, :298), so these are ordinary torch modules with
the same registration order as the reference's networks (curvature/lenet5.py:11-24,
curvature/resnet.py:24-201 with the 7x7/stride-2 ImageNet stem) -- ``model.modules()`` order is the
layer-indexing contract (tests/golden/g11_layer_tables.json).
PyTorch-ROCm runs their forward/backward; nothing here is on the accelerated path.
"""
from typing import List, Sequence, Tuple

import torch
from torch import nn


class Flatten(nn.Module):
    def forward(self, x):
        return x.view(x.size(0), -1)


def lenet5() -> nn.Sequential:
    """LeNet-5 variant of the reference (curvature/lenet5.py:11-24): 28x28 input, all layers biased."""
    return nn.Sequential(
        nn.Conv2d(1, 6, 5, padding=2), nn.ReLU(), nn.MaxPool2d(2, 2),
        nn.Conv2d(6, 16, 5), nn.ReLU(), nn.MaxPool2d(2, 2),
        Flatten(),
        nn.Linear(400, 120), nn.ReLU(),
        nn.Linear(120, 84), nn.ReLU(),
        nn.Linear(84, 10))


def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)


class _Residual(nn.Module):
    """Basic (two 3x3) or bottleneck (1x1, 3x3, 1x1) residual unit; stride sits on the 3x3 of the
    bottleneck (curvature/resnet.py:76) and on the first 3x3 of the basic block (:38)."""

    def __init__(self, cin: int, width: int, stride: int, bottleneck: bool):
        super().__init__()
        cout = width * (4 if bottleneck else 1)
        if bottleneck:
            self.conv1, self.bn1 = _conv(cin, width, 1), nn.BatchNorm2d(width)
            self.conv2, self.bn2 = _conv(width, width, 3, stride), nn.BatchNorm2d(width)
            self.conv3, self.bn3 = _conv(width, cout, 1), nn.BatchNorm2d(cout)
        else:
            self.conv1, self.bn1 = _conv(cin, width, 3, stride), nn.BatchNorm2d(width)
            self.conv2, self.bn2 = _conv(width, cout, 3), nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))
        self.bottleneck = bottleneck

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        if self.bottleneck:
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
        else:
            out = self.bn2(self.conv2(out))
        out = out + identity
        return self.relu(out)


class ResNet(nn.Module):
    def __init__(self, depths: Sequence[int], bottleneck: bool, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        cin = 64
        for stage, (depth, width) in enumerate(zip(depths, (64, 128, 256, 512))):
            units = []
            for u in range(depth):
                units.append(_Residual(cin, width, 2 if (u == 0 and stage > 0) else 1, bottleneck))
                cin = width * (4 if bottleneck else 1)
            setattr(self, f"layer{stage + 1}", nn.Sequential(*units))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(cin, num_classes)
        for mod in self.modules():          # curvature/resnet.py:145-150
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(self.avgpool(x).flatten(1))


def resnet18(num_classes: int = 1000) -> ResNet:
    return ResNet((2, 2, 2, 2), bottleneck=False, num_classes=num_classes)


def resnet50(num_classes: int = 1000) -> ResNet:
    return ResNet((3, 4, 6, 3), bottleneck=True, num_classes=num_classes)


class _GroupedBottleneck(nn.Module):
    """ResNeXt bottleneck (torchvision's Bottleneck with groups / width_per_group): 1x1, grouped 3x3 (stride here), 1x1."""

    def __init__(self, cin: int, planes: int, stride: int, groups: int, base_width: int):
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups
        cout = planes * 4
        self.conv1, self.bn1 = _conv(cin, width, 1), nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3, self.bn3 = _conv(width, cout, 1), nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNeXt(nn.Module):
    """ImageNet ResNeXt with torchvision's module registration order (grouped 3x3 convolutions in every unit)."""

    def __init__(self, depths: Sequence[int], groups: int, width_per_group: int, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        cin = 64
        for stage, (depth, planes) in enumerate(zip(depths, (64, 128, 256, 512))):
            units = []
            for u in range(depth):
                units.append(_GroupedBottleneck(cin, planes, 2 if (u == 0 and stage > 0) else 1, groups, width_per_group))
                cin = planes * 4
            setattr(self, f"layer{stage + 1}", nn.Sequential(*units))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(cin, num_classes)
        for mod in self.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(self.avgpool(x).flatten(1))


def resnext50_32x4d(num_classes: int = 1000) -> ResNeXt:
    return ResNeXt((3, 4, 6, 3), groups=32, width_per_group=4, num_classes=num_classes)


def _conv_bn_relu(cin: int, cout: int, k: int, stride: int = 1, groups: int = 1) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout),
                         nn.ReLU6(inplace=True))


class _InvertedResidual(nn.Module):
    """MobileNetV2 unit (torchvision's InvertedResidual): 1x1 expansion (t != 1), depthwise 3x3, linear 1x1."""

    def __init__(self, cin: int, cout: int, stride: int, expand: int):
        super().__init__()
        hidden = cin * expand
        self.use_res_connect = stride == 1 and cin == cout
        layers = [_conv_bn_relu(cin, hidden, 1)] if expand != 1 else []
        layers += [_conv_bn_relu(hidden, hidden, 3, stride, groups=hidden),
                   nn.Conv2d(hidden, cout, 1, bias=False), nn.BatchNorm2d(cout)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


class MobileNetV2(nn.Module):
    """MobileNetV2 (width 1.0) with torchvision's registration order: 17 depthwise 3x3 convolutions."""

    def __init__(self, num_classes: int = 1000):
        super().__init__()
        settings = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
        features = [_conv_bn_relu(3, 32, 3, 2)]
        cin = 32
        for t, c, n, s in settings:
            for i in range(n):
                features.append(_InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        features.append(_conv_bn_relu(cin, 1280, 1))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(nn.Dropout(0.2), nn.Linear(1280, num_classes))
        for mod in self.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode="fan_out")
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.ones_(mod.weight)
                nn.init.zeros_(mod.bias)
            elif isinstance(mod, nn.Linear):
                nn.init.normal_(mod.weight, 0, 0.01)
                nn.init.zeros_(mod.bias)

    def forward(self, x):
        x = self.features(x)
        x = nn.functional.adaptive_avg_pool2d(x, (1, 1)).flatten(1)
        return self.classifier(x)


def mobilenet_v2(num_classes: int = 1000) -> MobileNetV2:
    return MobileNetV2(num_classes)


class _DenseUnit(nn.Module):
    """BN-ReLU-Conv1x1 (to bn_size * growth channels) then BN-ReLU-Conv3x3 (to growth channels); the output is appended
    to the unit's input (Huang et al. 2017; the README's DenseNet-121 / 161 rows, README.rst:259-267)."""

    def __init__(self, cin: int, growth: int, bn_size: int):
        super().__init__()
        self.norm1, self.conv1 = nn.BatchNorm2d(cin), nn.Conv2d(cin, bn_size * growth, 1, bias=False)
        self.norm2, self.conv2 = nn.BatchNorm2d(bn_size * growth), nn.Conv2d(bn_size * growth, growth, 3, padding=1, bias=False)

    def forward(self, x):
        y = self.conv1(torch.relu(self.norm1(x)))
        y = self.conv2(torch.relu(self.norm2(y)))
        return torch.cat([x, y], 1)


class DenseNet(nn.Module):
    """ImageNet DenseNet-BC: 7x7 / stride-2 stem, dense blocks of `_DenseUnit`s joined by 1x1 transitions that halve the
    channels and the resolution.  Its layer geometries differ from a ResNet's in what matters to the factor build:
    1x1 convolutions whose input width grows by `growth` per unit (64 + 32 k, 96 + 48 k: most of them no multiple of
    128) and 3x3 convolutions with 128 / 192 input channels."""

    def __init__(self, growth: int, blocks: Sequence[int], init_features: int, bn_size: int = 4, num_classes: int = 1000):
        super().__init__()
        feats = [nn.Conv2d(3, init_features, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(init_features),
                 nn.ReLU(inplace=True), nn.MaxPool2d(3, stride=2, padding=1)]
        c = init_features
        for bi, depth in enumerate(blocks):
            for _ in range(depth):
                feats.append(_DenseUnit(c, growth, bn_size))
                c += growth
            if bi + 1 < len(blocks):
                feats += [nn.BatchNorm2d(c), nn.ReLU(inplace=True), nn.Conv2d(c, c // 2, 1, bias=False), nn.AvgPool2d(2, 2)]
                c //= 2
        feats.append(nn.BatchNorm2d(c))
        self.features = nn.Sequential(*feats)
        self.classifier = nn.Linear(c, num_classes)
        for mod in self.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight)
            elif isinstance(mod, nn.BatchNorm2d):
                nn.init.constant_(mod.weight, 1)
                nn.init.constant_(mod.bias, 0)

    def forward(self, x):
        x = torch.relu(self.features(x))
        return self.classifier(torch.nn.functional.adaptive_avg_pool2d(x, (1, 1)).flatten(1))


def densenet121(num_classes: int = 1000) -> DenseNet:
    return DenseNet(32, (6, 12, 24, 16), 64, num_classes=num_classes)


def densenet161(num_classes: int = 1000) -> DenseNet:
    return DenseNet(48, (6, 12, 36, 24), 96, num_classes=num_classes)


def dcgan_generator(nz: int = 100, ngf: int = 64, nc: int = 3) -> nn.Sequential:
    """DCGAN generator (Radford et al. 2016): a (N, nz, 1, 1) latent to an (N, nc, 64, 64) image.  The first layer is a
    ConvTranspose2d(kernel 4, stride 1, padding 0) on the 1x1 latent, the other four are (kernel 4, stride 2, padding 1)
    upsamplings; no biases, BatchNorm + ReLU between them, tanh at the end."""
    layers = [nn.ConvTranspose2d(nz, ngf * 8, 4, 1, 0, bias=False), nn.BatchNorm2d(ngf * 8), nn.ReLU(True)]
    c = ngf * 8
    for _ in range(3):
        layers += [nn.ConvTranspose2d(c, c // 2, 4, 2, 1, bias=False), nn.BatchNorm2d(c // 2), nn.ReLU(True)]
        c //= 2
    layers += [nn.ConvTranspose2d(c, nc, 4, 2, 1, bias=False), nn.Tanh()]
    return nn.Sequential(*layers)


def _double_conv(cin: int, cout: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True),
                         nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class UNet(nn.Module):
    """U-Net (Ronneberger et al. 2015) with padded convolutions: four 2x2 max-pool downsamplings, four
    ConvTranspose2d(C, C/2, kernel 2, stride 2) upsamplings (biased), skip concatenations, 1x1 classifier."""

    def __init__(self, in_channels: int = 3, num_classes: int = 2, width: int = 64):
        super().__init__()
        w = [width * 2 ** i for i in range(5)]
        self.inc = _double_conv(in_channels, w[0])
        self.down = nn.ModuleList([_double_conv(w[i], w[i + 1]) for i in range(4)])
        self.pool = nn.MaxPool2d(2)
        self.up = nn.ModuleList([nn.ConvTranspose2d(w[i + 1], w[i], 2, stride=2) for i in reversed(range(4))])
        self.dec = nn.ModuleList([_double_conv(2 * w[i], w[i]) for i in reversed(range(4))])
        self.outc = nn.Conv2d(w[0], num_classes, 1)

    def forward(self, x):
        skips = [self.inc(x)]
        for down in self.down:
            skips.append(down(self.pool(skips[-1])))
        y = skips.pop()
        for up, dec in zip(self.up, self.dec):
            y = dec(torch.cat([skips.pop(), up(y)], dim=1))
        return self.outc(y)


def unet(in_channels: int = 3, num_classes: int = 2, width: int = 64) -> UNet:
    return UNet(in_channels, num_classes, width)


def layer_table(model: nn.Module, input_chw: Tuple[int, int, int]) -> List[dict]:
    """[(index, name, kind, n, m, L, has_bias)] in ``model.modules()`` order for the selected layers.

    n = Cin*kh*kw (+1 with bias), m = Cout, L = output positions per sample."""
    names = {m: n for n, m in model.named_modules()}
    shapes = {}
    handles = []
    for mod in model.modules():
        if mod.__class__.__name__ in ("Conv2d", "Linear"):
            handles.append(mod.register_forward_hook(lambda m, i, o: shapes.__setitem__(m, tuple(o.shape))))
    was_training = model.training
    model.eval()
    with torch.no_grad():
        p = next(model.parameters())
        model(torch.zeros(1, *input_chw, dtype=p.dtype, device=p.device))
    model.train(was_training)
    for h in handles:
        h.remove()
    rows = []
    for mod in model.modules():
        kind = mod.__class__.__name__
        if kind not in ("Conv2d", "Linear"):
            continue
        bias = mod.bias is not None
        if kind == "Conv2d":
            n = mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1] + int(bias)
            m, L = mod.out_channels, shapes[mod][2] * shapes[mod][3]
        else:
            n, m, L = mod.in_features + int(bias), mod.out_features, 1
        rows.append({"index": len(rows), "name": names[mod], "kind": kind, "n": n, "m": m, "L": L,
                     "has_bias": bias})
    return rows
