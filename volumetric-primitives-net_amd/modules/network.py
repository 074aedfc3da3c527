"""modules/network of the reference: VPNetOneRes, VPNetTwoRes and SDNet (vpnet_one_resnet.py, vpnet_two_resnet.py,
sdnet.py), with the same attribute and `state_dict` names, so that a reference checkpoint loads with strict=True
(train_gcn.py:100-102, every test*.py).  The trunk is a ResNet-18: its convolutions are ATen's, and so is everything
around them by default; with `hip_conv` the 3x3 stride-1 convolutions of the chosen stages run on csrc/trunkconv.hip, with
`hip_conv_strided` the seven stride-2 ones (the stem, layerN.0.conv1, layerN.0.downsample.0) on csrc/trunkstride.hip (the
nn.Conv2d modules then only HOLD the weights); with `fused_norm=True` each batch norm, with the residual add and the ReLU that follow it, is one
op on csrc/trunknorm.hip (the nn.BatchNorm2d modules then only HOLD parameters and buffers), with `fused_pool` / `fused_tail` the
stem's max pool and the global average pool are part of the norm site before them; ResNet18.fold() makes the inference form
for a trunk that is not trained (eval mode under no_grad: train_gcn.py's frozen VPN, test.py): every batch norm folded into
the convolution before it, bias, residual add and ReLU in the convolution's epilogue on csrc/trunkfold.hip; the FC heads, the one part of the networks that is nothing but weight traffic, run on csrc/fcstack.hip: their
nn.Linear modules only HOLD the parameters, the forward hands the tensors to FcStackFunction, which also applies what
follows the last layer (restrict_range + split + restrict_volumes into packed rows, or SDNet's tanh).  GCNModel (gcn.py,
the refinement stage of train_gcn.py / test_gcn.py) is re-exported from modules/gcn.py, so that
`from modules.network import GCNModel` resolves."""
import torch
import torch.nn as nn

from .. import config
from ..ops import HeadPackFunction, FcStackFunction, BatchNormActFunction, BatchNormPoolFunction, BatchNormMeanFunction, Conv3x3Function, Conv2dFunction, conv2d_bias_act
from .gcn import GCNModel, GCNConv  # noqa: F401


def pack_head_outputs(volumes: torch.Tensor, rotates: torch.Tensor, translates: torch.Tensor,
                      is_sigmoid=config.IS_SIGMOID, clamp_min=config.VP_CLAMP_MIN, clamp_max=config.VP_CLAMP_MAX,
                      volume_restrict=config.VOLUME_RESTRICT) -> torch.Tensor:
    """restrict_range (:67-77) -> split (:36-38) -> restrict_volumes (:79-85) in one launch: raw head outputs
    volumes (B,3K), rotates (B,4K), translates (B,3K) -> packed parameters (B,K,10), differentiable."""
    return HeadPackFunction.apply(volumes, rotates, translates, is_sigmoid, clamp_min, clamp_max, volume_restrict)


def split_primitives(params: torch.Tensor):
    """Packed (B,K,10) -> the three python lists of K tensors (B,3), (B,4), (B,3) that the reference's model
    returns (:36-41) and train.py:105-120, :185 consume; views, no copy."""
    K = params.shape[1]
    return ([params[:, k, 0:3] for k in range(K)], [params[:, k, 3:7] for k in range(K)],
            [params[:, k, 7:10] for k in range(K)])


# ---- the trunk: torchvision's resnet18 by its parameter and buffer names (torchvision itself is not a dependency)

def batch_norm_act(x, bn: nn.BatchNorm2d, residual=None, relu=True):
    """relu?(bn(x) + residual?) in one op on csrc/trunknorm.hip, with the parameters, buffers, momentum, eps and mode of
    `bn`, which is not called: in training mode its running statistics and num_batches_tracked are updated in place on the
    device, as nn.BatchNorm2d does."""
    return BatchNormActFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                      residual, bn.training, bn.momentum, bn.eps, relu)


def batch_norm_relu_pool(x, bn: nn.BatchNorm2d):
    """max_pool2d(relu(bn(x)), 3, 2, 1) in one op on csrc/trunknorm.hip, with the parameters, buffers,
    momentum, eps and mode of `bn`, which is not called; the full-size activation is never written.  Training mode updates
    the running statistics and num_batches_tracked in place on the device, as nn.BatchNorm2d does."""
    return BatchNormPoolFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                       bn.training, bn.momentum, bn.eps)


def batch_norm_act_mean(x, bn: nn.BatchNorm2d, residual=None, relu=True):
    """(y, m) with y = relu?(bn(x) + residual?) and m = y.mean((2, 3)), the global average pool, in one op on
    csrc/trunknorm.hip, with the parameters, buffers, momentum, eps and mode of `bn`, which is not called.  y
    and what training mode updates in place are batch_norm_act's bit for bit; both outputs are differentiable."""
    return BatchNormMeanFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                       residual, bn.training, bn.momentum, bn.eps, relu)


def _is_tail_pool(pool):
    """AdaptiveAvgPool2d to 1x1, or SDNet's nn.Sequential that holds exactly one: the one pool the tail of
    csrc/trunknorm.hip holds."""
    if isinstance(pool, nn.Sequential) and len(pool) == 1:
        pool = pool[0]
    if not isinstance(pool, nn.AdaptiveAvgPool2d):
        return False
    size = pool.output_size
    return tuple(size) == (1, 1) if isinstance(size, (tuple, list)) else size == 1


def _is_stem_pool(pool):
    """MaxPool2d(3, 2, 1): the one pool csrc/trunknorm.hip holds."""
    def both(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (both(pool.kernel_size) == (3, 3) and both(pool.stride) == (2, 2) and both(pool.padding) == (1, 1) and
            both(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)


def conv3x3(x, weight):
    """conv2d(x, weight, stride 1, padding 1) for a (C_out, C_in, 3, 3) weight without bias, on csrc/trunkconv.hip: exact
    fp32 products on the f32-input MFMA, one summation order, differentiable in x and weight."""
    return Conv3x3Function.apply(x, weight)


def conv2d(x, weight, stride=1, padding=0):
    """conv2d(x, weight, stride, padding) for a (C_out, C_in, R, R) weight with R of 1, 3 or 7, without bias, on
    csrc/trunkstride.hip: exact fp32 products on the f32-input MFMA, one summation order, differentiable in x and weight.
    stride and padding are ints (both directions alike).  With a 3x3 weight, stride 1 and padding 1 it equals conv3x3 bit
    for bit."""
    return Conv2dFunction.apply(x, weight, stride, padding)


def fold_batch_norm(weight, bn: nn.BatchNorm2d):
    """(w', b') with conv2d(x, w') + b' = bn(conv2d(x, weight)) in eval mode: the norm's fixed scale
    s = gamma / sqrt(running_var + eps), formed in float64, multiplied into the rows of `weight` (C_out, C_in, R, R), and
    its shift b' = beta - running_mean s; both rounded to fp32 once.  On the tensors' device, no host synchronisation.  The
    mode of `bn` is not asked: the fold is the eval-mode norm.  A norm without affine parameters or without running
    statistics is refused."""
    if bn.weight is None or bn.bias is None:
        raise ValueError('fold_batch_norm: the norm has no affine parameters (affine=False)')
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError('fold_batch_norm: the norm has no running statistics (track_running_stats=False)')
    if weight.dim() != 4 or weight.shape[0] != bn.weight.shape[0]:
        raise ValueError('fold_batch_norm: weight must be (C_out, C_in, R, R) with C_out = %d, got %s' % (bn.weight.shape[0], tuple(weight.shape)))
    with torch.no_grad():
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return ((weight.double() * s.view(-1, 1, 1, 1)).float(), (bn.bias.double() - bn.running_mean.double() * s).float())


def _is_fold_conv(conv):
    """A convolution csrc/trunkfold.hip holds: square kernel of 1, 3 or 7, one stride and one padding, no bias."""
    k, p = conv.kernel_size, conv.padding
    return (k[0] == k[1] and k[0] in (1, 3, 7) and conv.stride[0] == conv.stride[1] and not isinstance(p, str) and p[0] == p[1] and
            conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros')


def _fold_act(x, conv, folded, residual=None, relu=True):
    """One folded site: `conv` gives the stride and the padding, `folded` = (w', b') the tensors."""
    return conv2d_bias_act(x, folded[0], folded[1], residual, conv.stride[0], conv.padding[0], relu)


def _use_fold(model):
    """The folded path is taken when a fold exists, the trunk is not in training mode and grad mode is off: autograd needs
    the unfolded graph."""
    return getattr(model, '_fold', None) is not None and not model.training and not torch.is_grad_enabled()


def _is_trunk_conv_strided(conv):
    """The trunk's convolutions with a stride: the 7x7 stem, the 3x3 layerN.0.conv1 and the 1x1 layerN.0.downsample.0."""
    k, p = conv.kernel_size, conv.padding
    return (k[0] == k[1] and k[0] in (1, 3, 7) and conv.stride[0] == conv.stride[1] and conv.stride[0] > 1 and
            not isinstance(p, str) and p[0] == p[1] and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and
            conv.padding_mode == 'zeros')


def _conv_strided(conv, x):
    """`conv` (a module _is_trunk_conv_strided accepts) on csrc/trunkstride.hip: the module only holds the weight."""
    return Conv2dFunction.apply(x, conv.weight, conv.stride[0], conv.padding[0])


def _is_trunk_conv3x3(conv):
    return (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1) and
            conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros')


TRUNK_STAGES = ('layer1', 'layer2', 'layer3', 'layer4')


def _hip_conv_stages(hip_conv):
    """hip_conv of ResNet18 -> the tuple of stage names whose 3x3 stride-1 convolutions leave ATen."""
    if isinstance(hip_conv, bool) or hip_conv is None:
        return TRUNK_STAGES if hip_conv else ()
    if isinstance(hip_conv, str):
        hip_conv = (hip_conv,)
    stages = tuple(hip_conv)
    for s in stages:
        if s not in TRUNK_STAGES:
            raise ValueError('hip_conv: %r is not one of %s' % (s, TRUNK_STAGES))
    return tuple(s for s in TRUNK_STAGES if s in stages)


class BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=1, fused_norm=False, hip_conv=False, hip_conv_strided=False):
        super().__init__()
        self.fused_norm = bool(fused_norm)
        self.hip_conv = bool(hip_conv)
        self.hip_conv_strided = bool(hip_conv_strided)
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))

    def _conv(self, conv, x):
        """`conv` on csrc/trunkconv.hip when this block's stage was chosen and it is a 3x3 stride-1 one, on
        csrc/trunkstride.hip when hip_conv_strided and it has a stride (the conv1 and the downsample of a stage's first
        block), else the module itself."""
        if self.hip_conv and _is_trunk_conv3x3(conv):
            return conv3x3(x, conv.weight)
        if self.hip_conv_strided and _is_trunk_conv_strided(conv):
            return _conv_strided(conv, x)
        return conv(x)

    def forward_tail(self, x):
        """forward with the global average pool: (relu(bn2(conv2(.)) + identity), its mean over (H, W)), the last site as
        one op on csrc/trunknorm.hip whatever fused_norm says."""
        if self.fused_norm:
            out = batch_norm_act(self._conv(self.conv1, x), self.bn1, relu=True)
            identity = x if self.downsample is None else batch_norm_act(self._conv(self.downsample[0], x), self.downsample[1], relu=False)
        else:
            out = self.relu(self.bn1(self._conv(self.conv1, x)))
            if self.downsample is None:
                identity = x
            elif self.hip_conv_strided and _is_trunk_conv_strided(self.downsample[0]):
                identity = self.downsample[1](_conv_strided(self.downsample[0], x))
            else:
                identity = self.downsample(x)
        return batch_norm_act_mean(self._conv(self.conv2, out), self.bn2, residual=identity, relu=True)

    def forward(self, x):
        if self.fused_norm:
            out = batch_norm_act(self._conv(self.conv1, x), self.bn1, relu=True)
            identity = x if self.downsample is None else batch_norm_act(self._conv(self.downsample[0], x), self.downsample[1], relu=False)
            return batch_norm_act(self._conv(self.conv2, out), self.bn2, residual=identity, relu=True)
        out = self.relu(self.bn1(self._conv(self.conv1, x)))
        out = self.bn2(self._conv(self.conv2, out))
        if self.downsample is None:
            return self.relu(out + x)
        if self.hip_conv_strided and _is_trunk_conv_strided(self.downsample[0]):
            return self.relu(out + self.downsample[1](_conv_strided(self.downsample[0], x)))
        return self.relu(out + self.downsample(x))


class ResNet18(nn.Module):
    """ResNet-18 (He et al. 2016) laid out as torchvision.models.resnet18: 122 state_dict entries, 11 689 512
    parameters, the `fc` 512 -> 1000 that the reference's models never call included.  Weights come from
    load_state_dict alone: nothing is ever downloaded.  fused_norm=True: the same modules under the same names (the
    same state_dict, loadable either way with strict=True), every norm / add / ReLU site on csrc/trunknorm.hip.
    hip_conv: True, False or an iterable of stage names out of ('layer1', 'layer2', 'layer3', 'layer4'): the 13 convolutions
    with kernel 3, stride 1, padding 1 of those stages run on csrc/trunkconv.hip, their nn.Conv2d modules only hold the
    weights; conv1 (7x7), the three stride-2 convolutions and the three 1x1 downsamples are not among them.
    hip_conv_strided=True: those seven (conv1, every layerN.0.conv1 and layerN.0.downsample[0] with stride 2) run on
    csrc/trunkstride.hip; with hip_conv=True as well no library convolution is left in the trunk, forward or backward.
    fused_pool=True: the stem's maxpool(relu(bn1(.))) is one op on csrc/trunknorm.hip (batch_norm_relu_pool) whatever
    fused_norm says; self.maxpool stays registered and is not called.
    fused_tail=True: layer4[1]'s relu(bn2(conv2(.)) + identity) and the global average pool are one op on csrc/trunknorm.hip
    (batch_norm_act_mean) whatever fused_norm says; self.avgpool stays registered and is not called.  The five keywords are
    independent; the state_dict is the same either way.
    fold() / unfold(): the inference form (every norm folded into its convolution, 20 launches of conv2d_bias_act on
    csrc/trunkfold.hip and the two pools), taken only in eval mode with grad mode off; see fold()."""

    def __init__(self, num_classes=1000, fused_norm=False, hip_conv=False, hip_conv_strided=False, fused_pool=False,
                 fused_tail=False):
        super().__init__()
        f = self.fused_norm = bool(fused_norm)
        self.fused_pool = bool(fused_pool)
        self.fused_tail = bool(fused_tail)
        g = self.hip_conv_strided = bool(hip_conv_strided)
        self.hip_conv = _hip_conv_stages(hip_conv)
        h = {s: s in self.hip_conv for s in TRUNK_STAGES}
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        k = dict(fused_norm=f, hip_conv=h['layer1'], hip_conv_strided=g)
        self.layer1 = nn.Sequential(BasicBlock(64, 64, **k), BasicBlock(64, 64, **k))
        k = dict(fused_norm=f, hip_conv=h['layer2'], hip_conv_strided=g)
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2, **k), BasicBlock(128, 128, **k))
        k = dict(fused_norm=f, hip_conv=h['layer3'], hip_conv_strided=g)
        self.layer3 = nn.Sequential(BasicBlock(128, 256, 2, **k), BasicBlock(256, 256, **k))
        k = dict(fused_norm=f, hip_conv=h['layer4'], hip_conv_strided=g)
        self.layer4 = nn.Sequential(BasicBlock(256, 512, 2, **k), BasicBlock(512, 512, **k))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)
        self._fold = None                              # fold(): the inference form, a plain attribute
        for m in self.modules():                       # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def _conv1(self, x):
        """The 7x7 stem convolution: on csrc/trunkstride.hip with hip_conv_strided, else the module itself."""
        return _conv_strided(self.conv1, x) if self.hip_conv_strided and _is_trunk_conv_strided(self.conv1) else self.conv1(x)

    def _stem_tail(self, x):
        """maxpool(relu(bn1(x))) of the stem convolution's output, by the form the keywords chose."""
        if self.fused_pool:
            if not _is_stem_pool(self.maxpool):
                raise ValueError('fused_pool: csrc/trunknorm.hip holds MaxPool2d(3, 2, 1) only, self.maxpool is %r' % (self.maxpool,))
            return batch_norm_relu_pool(x, self.bn1)
        if self.fused_norm:
            return self.maxpool(batch_norm_act(x, self.bn1, relu=True))
        return self.maxpool(self.relu(self.bn1(x)))

    def _stem(self, x):
        return self._stem_tail(self._conv1(x))

    def _check_tail_pool(self):
        if not _is_tail_pool(self.avgpool):
            raise ValueError('fused_tail: csrc/trunknorm.hip holds AdaptiveAvgPool2d to 1x1 only, self.avgpool is %r' % (self.avgpool,))

    def _layer4_tail(self, x):
        """(layer4(x), its global average pool [B,512]) with fused_tail: layer4[1]'s last site writes both."""
        self._check_tail_pool()
        for block in self.layer4[:-1]:
            x = block(x)
        return self.layer4[-1].forward_tail(x)

    def _fold_sites(self):
        """The 20 (convolution, norm) sites in the order the folded forward calls them: the stem, then per block conv1,
        the downsample where there is one, conv2."""
        sites = [(self.conv1, self.bn1)]
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for block in layer:
                sites.append((block.conv1, block.bn1))
                if block.downsample is not None:
                    sites.append((block.downsample[0], block.downsample[1]))
                sites.append((block.conv2, block.bn2))
        return sites

    @staticmethod
    def _fold_sources(sites):
        """The tensors a fold of `sites` reads."""
        return [t for conv, bn in sites for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)]

    def fold(self):
        """The inference form of the trunk: every batch norm folded into the convolution before it
        (fold_batch_norm), from the modules as they stand.  While the fold exists, the trunk is in eval mode and grad mode
        is off, forward and the models' extract_feature run 20 conv2d_bias_act on csrc/trunkfold.hip (bias, residual add
        and ReLU in the convolution's epilogue) and the two pools; the five keywords select nothing there.  In any other
        setting the trunk runs as without a fold.  The folded tensors are a plain attribute: no parameter, buffer or
        module is registered, the state_dict is unchanged.  The fold remembers the version of every tensor it read; a
        forward after one of them changed (load_state_dict, an optimiser step, .to(device)) raises and asks for fold()
        again.  Returns self."""
        sites = self._fold_sites()
        for conv, _bn in sites:
            if not _is_fold_conv(conv):
                raise ValueError('fold: csrc/trunkfold.hip holds square kernels of 1, 3 or 7 without bias only, got %r' % (conv,))
        pairs = [fold_batch_norm(conv.weight, bn) for conv, bn in sites]
        self._fold = (pairs, [(t, t._version) for t in self._fold_sources(sites)])
        return self

    def unfold(self):
        """Drop the fold: the trunk runs by its modules and keywords again.  Returns self."""
        self._fold = None
        return self

    def _fold_pairs(self):
        """The 20 (w', b') of the fold, or RuntimeError when a tensor it was made from has changed since (another tensor,
        another version, another device): host integers only, no synchronisation."""
        pairs, seen = self._fold
        now = self._fold_sources(self._fold_sites())
        if len(now) != len(seen) or any(t is not u or t._version != v or t.device != pairs[0][0].device for t, (u, v) in zip(now, seen)):
            raise RuntimeError('ResNet18: the fold is stale (a parameter or running statistic changed after fold(), e.g. by '
                               'load_state_dict, an optimiser step or a move to another device): call fold() again')
        return pairs

    def _folded_maps(self, x):
        """The four residual stages' outputs on the folded path."""
        pairs = iter(self._fold_pairs())
        out = self.maxpool(_fold_act(x, self.conv1, next(pairs)))
        maps = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for block in layer:
                mid = _fold_act(out, block.conv1, next(pairs))
                identity = out if block.downsample is None else _fold_act(out, block.downsample[0], next(pairs), relu=False)
                out = _fold_act(mid, block.conv2, next(pairs), residual=identity)
            maps.append(out)
        return maps

    def forward(self, x):
        if _use_fold(self):
            return self.fc(torch.flatten(self.avgpool(self._folded_maps(x)[3]), 1))
        x = self.layer3(self.layer2(self.layer1(self._stem(x))))
        if self.fused_tail:
            return self.fc(self._layer4_tail(x)[1])
        return self.fc(torch.flatten(self.avgpool(self.layer4(x)), 1))


def _trunk_maps(model, imgs):
    """conv1 .. layer4 of a trunk (extract_feature of the three models): the four residual stages' outputs.  A folded
    trunk in eval mode with grad mode off (ResNet18.fold) forms them on csrc/trunkfold.hip."""
    if _use_fold(model):
        return model._folded_maps(imgs)
    stem = model._conv1(imgs) if getattr(model, 'hip_conv_strided', False) else model.conv1(imgs)
    if hasattr(model, '_stem_tail'):                      # ResNet18: by the form its keywords chose
        out = model._stem_tail(stem)
    else:
        out = model.maxpool(model.relu(model.bn1(stem)))
    l1 = model.layer1(out)
    l2 = model.layer2(l1)
    l3 = model.layer3(l2)
    return [l1, l2, l3, model.layer4(l3)]


def _trunk_features(model, imgs, pool=None):
    """(maps, feats): the four residual stages' outputs as _trunk_maps gives them, and the global average pool of the last
    one as [B,512].  `pool`: the pool of the model that owns the trunk (default: the trunk's own avgpool).  A trunk with
    fused_tail forms feats in layer4's last site: no pool is called, and one that is not the global average is refused
    before anything runs.  For any other trunk feats is pool(maps[3]), flattened."""
    pool = model.avgpool if pool is None else pool
    if _use_fold(model) or not getattr(model, 'fused_tail', False):      # the folded path ends in the owner's pool too
        maps = _trunk_maps(model, imgs)
        out = pool(maps[3])
        return maps, out.view(out.size(0), -1)
    if not _is_tail_pool(pool):
        raise ValueError('fused_tail: csrc/trunknorm.hip holds AdaptiveAvgPool2d to 1x1 only, the pool is %r' % (pool,))
    model._check_tail_pool()
    stem = model._conv1(imgs) if model.hip_conv_strided else model.conv1(imgs)
    l1 = model.layer1(model._stem_tail(stem))
    l2 = model.layer2(l1)
    l3 = model.layer3(l2)
    l4, feats = model._layer4_tail(l3)
    return [l1, l2, l3, l4], feats


# ---- the heads

def make_linear(output_dim, is_dropout=config.IS_DROPOUT, feat=512, hidden=1024):
    """_make_linear of the reference (vpnet_one_resnet.py:87-107): five nn.Linear, an nn.Dropout() after each of the
    first four when is_dropout (so the Linear indices are 0,2,4,6,8)."""
    mods, width = [], feat
    for l in range(5):
        mods.append(nn.Linear(width, hidden if l < 4 else output_dim))
        width = hidden
        if is_dropout and l < 4:
            mods.append(nn.Dropout())
    return nn.Sequential(*mods)


class FcHeads(nn.Module):
    """Owner of one or more FC heads.  The heads are nn.Sequential of nn.Linear (and nn.Dropout) exactly as the
    reference lays them out, registered under the reference's names, so state_dict keys match; run_heads never calls
    those modules: it hands their tensors to FcStackFunction (one launch per layer for all heads).  Used directly
    (`FcHeads({'volume_fc': 48, ...})`) or as the base of the three models."""

    def __init__(self, heads=None, is_dropout=config.IS_DROPOUT, feat=512, hidden=1024, seed=0):
        super().__init__()
        self._head_paths = []
        self._is_dropout = bool(is_dropout)
        self._fc_seed, self._fc_calls = int(seed), 0
        for name, out in (heads or {}).items():
            setattr(self, name, make_linear(out, is_dropout, feat, hidden))
            self._head_paths.append(name)

    def head_linears(self):
        """Per head, its nn.Linear modules in order."""
        return [[m for m in self.get_submodule(p) if isinstance(m, nn.Linear)] for p in self._head_paths]

    def run_heads(self, inputs, epilogue='none', masks=None, seed=None, **rule):
        """inputs: one tensor (B,feat) per head (the same tensor may be given several times).  Dropout applies in
        training mode where the heads were built with it: `masks` (per head, per layer 0..L-2, uint8 (B,out)) selects
        explicit keep masks, otherwise Philox draws them from `seed`: an int (default: the module's seed plus the number
        of calls so far, so every eager step draws anew), or a CUDA int64 tensor of one element that the kernels read, the
        form for a captured graph: bump it on the stream between steps (`seed.add_(1)` inside the capture, after the
        backward) and every replay draws anew.  It must not change between a forward and its backward."""
        lin = self.head_linears()
        G, L = len(lin), len(lin[0])
        assert len(inputs) == G and all(len(h) == L for h in lin)
        cfg = dict(G=G, L=L, epilogue=epilogue, dropout=None, **rule)
        extra = []
        if self._is_dropout and self.training and L > 1:
            cfg['p'] = next(m.p for m in self.get_submodule(self._head_paths[0]) if isinstance(m, nn.Dropout))
            if masks is not None:
                cfg['dropout'] = 'mask'
                extra = [m for head in masks for m in head]
            else:
                cfg['dropout'] = 'philox'
                if seed is None:
                    seed = self._fc_seed + self._fc_calls
                    self._fc_calls += 1
                cfg['seed'] = seed
        params = [t for head in lin for m in head for t in (m.weight, m.bias)]
        return FcStackFunction.apply(cfg, *inputs, *params, *extra)


class _VPNet(FcHeads):
    """What VPNetOneRes and VPNetTwoRes share: the three heads and the range rules.  The constructor arguments stand in
    for the reference's config constants (config.py:22-26, :36)."""

    def __init__(self, vp_num, is_sigmoid, is_dropout, clamp_min, clamp_max, volume_restrict, hidden, feat, seed):
        super().__init__(None, is_dropout, feat, hidden, seed)
        self._vp_num = int(vp_num)
        self._rule = dict(is_sigmoid=bool(is_sigmoid), clamp_min=float(clamp_min), clamp_max=float(clamp_max),
                          volume_restrict=tuple(float(r) for r in volume_restrict))
        self.avgpool = nn.AdaptiveAvgPool2d(output_size=(1, 1))
        self.volume_fc = make_linear(3 * self._vp_num, is_dropout, feat, hidden)
        self.rotate_fc = make_linear(4 * self._vp_num, is_dropout, feat, hidden)
        self.translate_fc = make_linear(3 * self._vp_num, is_dropout, feat, hidden)
        self._head_paths = ['volume_fc', 'rotate_fc', 'translate_fc']

    @staticmethod
    def restrict_range(volumes, rotates, translates, is_sigmoid=config.IS_SIGMOID, clamp_min=config.VP_CLAMP_MIN,
                       clamp_max=config.VP_CLAMP_MAX):
        """:67-77 on raw head outputs (B,3K), (B,4K), (B,3K), through the head kernel (GPU only).  A staticmethod as in
        the reference, which reads the config constants; here they are the defaults of the keyword arguments."""
        p = pack_head_outputs(volumes, rotates, translates, is_sigmoid, clamp_min, clamp_max, (1.0, 1.0, 1.0))
        B = p.shape[0]
        return p[:, :, 0:3].reshape(B, -1), p[:, :, 3:7].reshape(B, -1), p[:, :, 7:10].reshape(B, -1)

    @staticmethod
    def restrict_volumes(volumes, volume_restrict=config.VOLUME_RESTRICT):
        """:79-85 on a list of (B,3) tensors, out of place (the reference writes into views of a split, which autograd
        refuses).  The model's own forward does this inside the heads' last launch instead."""
        r = volumes[0].new_tensor([float(v) for v in volume_restrict])
        return [v / r for v in volumes]


class VPNetOneRes(_VPNet):
    """vpnet_one_resnet.py: one ResNet-18, three heads.  forward(imgs) -> (volumes, rotates, translates,
    perceptual_features, features) as the reference; forward_packed(imgs) -> (params (B,K,10), perceptual_features,
    features), the form the sampler, the raster and the losses of this package read."""

    def __init__(self, vp_num=config.VP_NUM, is_sigmoid=config.IS_SIGMOID, is_dropout=config.IS_DROPOUT,
                 clamp_min=config.VP_CLAMP_MIN, clamp_max=config.VP_CLAMP_MAX, volume_restrict=config.VOLUME_RESTRICT,
                 hidden=1024, feat=512, trunk=None, seed=0):
        super().__init__(vp_num, is_sigmoid, is_dropout, clamp_min, clamp_max, volume_restrict, hidden, feat, seed)
        self.resnet = ResNet18() if trunk is None else trunk

    def extract_feature(self, imgs):
        maps, feats = _trunk_features(self.resnet, imgs, self.avgpool)
        return feats, maps

    def fix_volume_weight(self):
        for p in self.volume_fc.parameters():
            p.requires_grad = False

    def forward_packed(self, imgs, masks=None, seed=None):
        features, perceptual_features = self.extract_feature(imgs)
        params = self.run_heads([features, features, features], 'vp_pack', masks, seed, **self._rule)
        return params, perceptual_features, features

    def forward(self, imgs):
        params, perceptual_features, features = self.forward_packed(imgs)
        volumes, rotates, translates = split_primitives(params)
        return volumes, rotates, translates, perceptual_features, features


class VPNetTwoRes(_VPNet):
    """vpnet_two_resnet.py: one ResNet-18 for the volumes, one for rotation and translation."""

    def __init__(self, vp_num=config.VP_NUM, is_sigmoid=config.IS_SIGMOID, is_dropout=config.IS_DROPOUT,
                 clamp_min=config.VP_CLAMP_MIN, clamp_max=config.VP_CLAMP_MAX, volume_restrict=config.VOLUME_RESTRICT,
                 hidden=1024, feat=512, trunk=None, seed=0):
        super().__init__(vp_num, is_sigmoid, is_dropout, clamp_min, clamp_max, volume_restrict, hidden, feat, seed)
        vt, tt = (ResNet18(), ResNet18()) if trunk is None else trunk          # trunk: a pair (volume, transform)
        self.volume_resnet = vt
        self.transform_resnet = tt

    def extract_feature(self, model, imgs):
        return _trunk_features(model, imgs, self.avgpool)[1]

    def fix_volume_weight(self):
        for p in self.volume_resnet.parameters():
            p.requires_grad = False
        for p in self.volume_fc.parameters():
            p.requires_grad = False

    def forward_packed(self, imgs, masks=None, seed=None):
        vf = self.extract_feature(self.volume_resnet, imgs)
        tf = self.extract_feature(self.transform_resnet, imgs)
        return self.run_heads([vf, tf, tf], 'vp_pack', masks, seed, **self._rule)

    def forward(self, imgs):
        return split_primitives(self.forward_packed(imgs))


class SDNet(FcHeads):
    """sdnet.py: the offsets of the 386 sphere vertices, tanh-bounded.  `_model` is the trunk with `avgpool` replaced
    and `deform` attached, as the reference does; `deform.5` is the nn.Tanh it ends in (no parameters): the heads'
    last launch applies it."""

    def __init__(self, vertex_num=386, hidden=1024, feat=512, trunk=None):
        super().__init__()
        self._vertex_num = int(vertex_num)
        self._model = ResNet18() if trunk is None else trunk
        self._model.avgpool = nn.Sequential(nn.AdaptiveAvgPool2d(output_size=(1, 1)))
        self._model.deform = nn.Sequential(*make_linear(self._vertex_num * 3, False, feat, hidden), nn.Tanh())
        self._head_paths = ['_model.deform']

    def extract_feature(self, imgs):
        return _trunk_features(self._model, imgs)[1]

    def forward(self, imgs):
        offsets = self.run_heads([self.extract_feature(imgs)], 'tanh')
        return offsets.view(imgs.size(0), self._vertex_num, 3)
