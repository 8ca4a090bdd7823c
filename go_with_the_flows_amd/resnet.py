"""Image encoder of the single-view-reconstruction model: a 4-channel ResNet-18 with an fc -> fc_bn -> ReLU head.

Same function, constructor arguments, attribute names and ``state_dict`` keys (in order) as the reference's
lib/networks/resnet.py:9-224 (``resnet18``, ``ResNet``, ``BasicBlock``), so a reference checkpoint loads with strict=True.
Written with stock ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.Linear`` / ``nn.BatchNorm1d``.

Two paths, the split the PointNet encoder had before its training kernels:
* eval mode (``model.eval()``), fp32 on a HIP device, 4 input channels, H and W >= 32, no autograd wanted: the HIP kernels of
  csrc/gwtf_resnet.hip (implicit-GEMM convolutions on the fp32 matrix cores with every BatchNorm folded in, split-K with a
  fixed-order reduction at small batch, max-pool, the head in one launch);
* train mode, or whenever a gradient must flow through the encoder: the plain torch modules (library convolutions, batch
  statistics, autograd).  With the class attribute ``ResNet.train_norm = 'hip'`` (default ``'library'``) a train-mode call keeps the
  library convolutions but runs every BatchNorm2d with the ReLU, residual add and stem max-pool behind it through the fused
  kernels of csrc/gwtf_norm2d.hip (norm2d.norm_act_2d), forward and backward; the head stays on the modules.  After
  ``nn.SyncBatchNorm.convert_sync_batchnorm`` in a data-parallel run the same path takes its batch statistics over the images of all
  ranks (one all-reduce of the float64 sums per layer and direction; the head on the gathered rows).  With ``ResNet.train_conv =
  'hip'`` as well (default ``'library'``; it needs ``train_norm = 'hip'``) the 20 convolutions of that path run on
  csrc/gwtf_conv2d.hip (conv2d.conv2d), forward, input gradient and weight gradient: no library call between the image and the
  pooled features, exact fp32 products, no atomics.  It is off by default: DESIGN section 8 item 6 has the per-layer standing
  against the library.  Convolutions have no collectives, so a data-parallel run needs nothing more.
``forward_torch`` runs the module graph on any device and dtype (the CPU float64 evaluation the tests compare against).
An eval-mode call that the kernels cannot take (CPU tensor, dtype other than float32, channels other than 4, images under
32 x 32) raises GwtfError: there is no fallback.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import GwtfError, _ptr, _stream, check
from .conv2d import conv2d
from .norm2d import norm_act_2d


def _conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        if groups != 1 or base_width != 64:
            raise ValueError('BasicBlock only supports groups=1 and base_width=64')
        if dilation > 1:
            raise NotImplementedError('Dilation > 1 not supported in BasicBlock')
        self.conv1 = _conv3x3(inplanes, planes, stride)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3x3(planes, planes)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        y = y + (x if self.downsample is None else self.downsample(x))
        return self.relu(y)


def _conv(conv, x, how='library'):
    if how == 'hip':
        return conv2d(x, conv)
    return F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)


class ResNet(nn.Module):
    train_norm = 'library'      # 'hip': train-mode BatchNorm2d (+ ReLU, residual, stem pool) on csrc/gwtf_norm2d.hip; not in state_dict
    train_conv = 'library'      # 'hip': the convolutions of the train_norm = 'hip' path on csrc/gwtf_conv2d.hip; not in state_dict

    def __init__(self, block, layers, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        self._norm_layer = norm_layer
        self.inplanes, self.dilation = 64, 1
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError('replace_stride_with_dilation should be None or a 3-element tuple, '
                             f'got {replace_stride_with_dilation}')
        self.groups, self.base_width = groups, width_per_group
        self.num_classes = num_classes
        self.conv1 = nn.Conv2d(4, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=replace_stride_with_dilation[0])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=replace_stride_with_dilation[1])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=replace_stride_with_dilation[2])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        self.fc_bn = nn.BatchNorm1d(num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, BasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)
        self._packed = None
        self._stamp = None
        self._hip_ok = block is BasicBlock and list(layers) == [2, 2, 2, 2] and groups == 1 and width_per_group == 64 \
            and not any(replace_stride_with_dilation) and norm_layer is nn.BatchNorm2d

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False):
        norm_layer = self._norm_layer
        downsample = None
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                norm_layer(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation,
                                norm_layer=norm_layer))
        return nn.Sequential(*layers)

    # ---- the module graph (train mode, autograd, and the CPU / float64 evaluation) ----
    def forward_torch(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = torch.flatten(self.avgpool(x), 1)
        return self.relu(self.fc_bn(self.fc(x)))

    def forward_train_hip(self, x):
        """The train-mode module graph with the fused BatchNorm2d kernels and the library's convolutions or, with train_conv =
        'hip', those of csrc/gwtf_conv2d.hip; same parameters, buffers and running-statistics updates as forward_torch in train
        mode."""
        if not self._hip_ok:
            raise GwtfError("train_norm='hip' covers resnet18 (BasicBlock x [2,2,2,2], BatchNorm2d) only")
        how = self._train_conv()
        x = norm_act_2d(_conv(self.conv1, x, how), self.bn1, pool=True)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                y = norm_act_2d(_conv(blk.conv1, x, how), blk.bn1)
                r = x if blk.downsample is None else norm_act_2d(_conv(blk.downsample[0], x, how), blk.downsample[1], relu=False)
                x = norm_act_2d(_conv(blk.conv2, y, how), blk.bn2, residual=r)
        return self._head_train(torch.flatten(self.avgpool(x), 1))

    def _train_conv(self):
        """train_conv, checked against train_norm: the HIP convolutions exist on the fused-norm path only."""
        if self.train_conv not in ('library', 'hip'):
            raise GwtfError(f"train_conv must be 'library' or 'hip', got {self.train_conv!r}")
        if self.train_conv == 'hip' and self.train_norm != 'hip':
            raise GwtfError(f"train_conv='hip' needs train_norm='hip' (got train_norm={self.train_norm!r}): the HIP convolutions run "
                            'inside forward_train_hip')
        return self.train_conv

    def _head_train(self, x):
        """fc -> fc_bn -> ReLU on the pooled rows.  In a synchronised data-parallel run (fc_bn a SyncBatchNorm) every rank evaluates
        the head on the pooled rows of ALL ranks and keeps its own (dist.gather_rows, as the per-shape heads do): fc_bn needs no
        collective of its own and every rank leaves the same running statistics."""
        from .dist import gather_rows, syncs_statistics
        bn = self.fc_bn
        if not syncs_statistics([bn]):
            return self.relu(bn(self.fc(x)))
        if bn.momentum is None or not bn.track_running_stats:
            raise GwtfError('the synchronised head takes an fc_bn with a momentum that tracks running statistics')
        rows = x.shape[0]
        x, lay = gather_rows(x)
        h = F.batch_norm(self.fc(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        return F.relu(h[lay.row0:lay.row0 + rows])

    # ---- packed weights (BatchNorm folded in float64 on the host), cached per parameter version ----
    def invalidate_packed_weights(self):
        self._packed = None
        self._src = None

    def train(self, mode=True):
        self._packed = None
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def _convs(self):
        """(conv, bn, downsample conv, downsample bn) in the packed order: stem, then conv1 / conv2 of every block."""
        out = [(self.conv1, self.bn1, None, None)]
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                out.append((blk.conv1, blk.bn1, None, None))
                ds = blk.downsample
                out.append((blk.conv2, blk.bn2, ds[0] if ds is not None else None, ds[1] if ds is not None else None))
        return out

    def _sources(self):
        if getattr(self, '_src', None) is None or self._packed is None:
            self._src = [t for t in self.state_dict(keep_vars=True).values() if t.dtype.is_floating_point]
        return self._src

    @staticmethod
    def _fold(bn):
        s = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
        return s, bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * s

    def _pack_host(self):
        """The packed arena of include/gwtf.h (gwtf_resnet_forward), float64 folds rounded once to fp32."""
        parts = []
        for conv, bn, dconv, dbn in self._convs():
            s, shift = self._fold(bn)
            w = conv.weight.detach().double().cpu()
            cout = w.shape[0]
            w = (w * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(cout, -1)
            if dconv is not None:
                ds, dshift = self._fold(dbn)
                w = torch.cat([w, dconv.weight.detach().double().cpu().reshape(cout, -1) * ds[:, None]], dim=1)
                shift = shift + dshift
            kp = (w.shape[1] + 15) // 16 * 16
            if kp != w.shape[1]:
                w = torch.cat([w, w.new_zeros(cout, kp - w.shape[1])], dim=1)
            parts += [w.reshape(-1), shift]
        s, _ = self._fold(self.fc_bn)
        bn = self.fc_bn
        parts.append((self.fc.weight.detach().double().cpu() * s[:, None]).reshape(-1))
        parts.append((self.fc.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu()) * s
                     + bn.bias.detach().double().cpu())
        return torch.cat(parts).float()

    def packed(self):
        src = self._sources()
        stamp = tuple((t.data_ptr(), t._version) for t in src)
        if self._packed is None or stamp != self._stamp:
            dev = self.conv1.weight.device
            host = self._pack_host()
            if host.numel() != _lib.lib().gwtf_resnet_packed_floats(self.num_classes):
                raise GwtfError('image encoder packed arena size mismatch')
            self._packed, self._stamp = host.to(dev), stamp
        return self._packed

    def _needs_graph(self, x):
        return self.training or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))

    def forward_hip(self, x, tune=0):
        """(B,4,H,W) fp32 HIP tensor -> (B,num_classes) through csrc/gwtf_resnet.hip (eval-mode BatchNorm)."""
        if not self._hip_ok:
            raise GwtfError('the HIP image encoder covers resnet18 (BasicBlock x [2,2,2,2], BatchNorm2d) only')
        if x.dim() != 4 or x.shape[1] != 4:
            raise GwtfError(f'image encoder input must be (B,4,H,W); got {tuple(x.shape)}')
        x = x.contiguous()
        _ptr(x, 'images')
        B, _, H, W = x.shape
        if B < 1 or H < 32 or W < 32:
            raise GwtfError(f'image encoder input must have B >= 1 and H, W >= 32; got {tuple(x.shape)}')
        L = _lib.lib()
        n_work = L.gwtf_resnet_work_floats(B, H, W, int(tune))
        if n_work == 0:
            raise GwtfError(f'image encoder: unsupported size {tuple(x.shape)} or tune word {tune:#x}')
        packed = self.packed()
        if packed.device != x.device:
            raise GwtfError(f'images on {x.device}, encoder weights on {packed.device}')
        out = torch.empty(B, self.num_classes, device=x.device, dtype=torch.float32)
        work = torch.empty(n_work, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            check(L.gwtf_resnet_forward(_ptr(x, 'images'), _ptr(packed, 'packed'), _ptr(out, 'out'), _ptr(work, 'work'),
                                        B, H, W, self.num_classes, int(tune), _stream(x)))
        return out

    def forward(self, x):
        if self._needs_graph(x):
            if self.train_norm not in ('library', 'hip'):
                raise GwtfError(f"train_norm must be 'library' or 'hip', got {self.train_norm!r}")
            self._train_conv()
            if self.train_norm == 'hip' and not self._hip_ok:
                raise GwtfError("train_norm='hip' covers resnet18 (BasicBlock x [2,2,2,2], BatchNorm2d) only")
            if not x.is_cuda:
                raise GwtfError(f'images must live on a HIP device (got {x.device}); forward_torch evaluates the module '
                                'graph anywhere')
            # eval mode with autograd keeps the library graph: the fused kernels compute batch statistics
            return self.forward_train_hip(x) if self.train_norm == 'hip' and self.training else self.forward_torch(x)
        return self.forward_hip(x)


def resnet18(pretrained=False, progress=True, **kwargs):
    """ResNet-18 with a 4-channel stem and the fc -> fc_bn -> ReLU head (reference resnet.py:214-224; no pretrained weights)."""
    if pretrained:
        raise ValueError('pretrained weights are not available: load a checkpoint with load_state_dict')
    return ResNet(BasicBlock, [2, 2, 2, 2], **kwargs)
