"""Host only: every weight pack follows ONE rule -- components.mlp.generation, the device and the version of every tensor of the module.

Per cached pack of the package: the same object on a repeated call; a new pack, bit-equal to a freshly constructed module's, after an in-place update
of any parameter and of any buffer the pack reads; no rebuild after an update of a buffer it does not read; a rebuild after load_state_dict and after
module.double().float(); a deepcopy that starts empty and is right with no further call; one object for two threads.  Nothing here touches a device
(SAModule._fused_pack asks the built library which edge MLPs gn_sa_fused takes, as tests/test_host_cpu.py loads it)."""
import copy
import threading

import pytest
import torch

from garmentnets_amd import autograd as A, ops
from garmentnets_amd.components import unet3d as U
from garmentnets_amd.components.mlp import MLP, HipLinear, generation, param_cache
from garmentnets_amd.components.pointnet2 import SAModule
from garmentnets_amd.networks.conv_implicit_wnf import ImplicitWNFDecoder
from garmentnets_amd.optim import FusedAdam


def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in list(module.parameters()) + [b for b in module.buffers() if b.dtype.is_floating_point]:
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    return module.eval()


def _leaves(pack):
    """every tensor of a pack, in a fixed order (tuples, lists, SplitPack / DecoderPack / SaFusedPack objects walked through)"""
    if torch.is_tensor(pack):
        return [pack]
    if isinstance(pack, (tuple, list)):
        return [t for p in pack for t in _leaves(p)]
    if isinstance(pack, dict):
        return [t for k in sorted(pack) for t in _leaves(pack[k])]
    fields = getattr(pack, "__dict__", None) or {k: getattr(pack, k) for k in getattr(pack, "__slots__", ())}
    return [t for k in sorted(fields) for t in _leaves(fields[k])]


def _same(a, b):
    la, lb = _leaves(a), _leaves(b)
    return len(la) == len(lb) > 0 and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(la, lb))


_LAY = U._Layout(((24,), (32,), 32))


def _conv(padded=False):
    conv = U.SingleConv(24 if padded else 32, 24 if padded else 32)
    if padded:
        conv.in_real = (24,)
    return conv


def _final():
    fc = U.FinalConv1x1(24, 128, 1)
    fc.in_stored = 32
    return fc


def _decoder():
    return ImplicitWNFDecoder((128, 256, 256, 1))


_FINAL = _randomise(_final(), 99)


def _sa():
    return SAModule(0.5, 0.2, MLP([3, 64, 64, 128]))


# name -> (constructor of the module whose tensors the pack reads, the pack getter, whether BatchNorm running statistics are read)
PACKS = {
    "MLPStack.packed": (lambda: MLP([6, 16, 8]), lambda m: m.packed(), True),
    "HipLinear.packed": (lambda: HipLinear(6, 5), lambda m: m.packed(), False),
    "SingleConv.packed": (_conv, lambda m: m.packed(), False),
    "SingleConv.weight_pack(fp32)": (_conv, lambda m: m.weight_pack("fp32", None), False),
    "SingleConv.weight_pack(fp32, padded)": (lambda: _conv(True), lambda m: m.weight_pack("fp32", _LAY), False),
    "SingleConv.weight_pack(bwd_data)": (lambda: _conv(True), lambda m: m.weight_pack("bwd_data", _LAY), False),
    "SingleConv.weight_pack(padded_weight)": (lambda: _conv(True), lambda m: m.weight_pack("padded_weight", _LAY), False),
    "FinalConv1x1.packed": (_final, lambda m: m.packed(), False),
    "ImplicitWNFDecoder.packed": (_decoder, lambda m: m.packed(), True),
    "ImplicitWNFDecoder.folded_pack": (_decoder, lambda m: m.folded_pack(_FINAL), True),
    "SAModule._fused_pack": (_sa, lambda m: m._fused_pack(), True),
}


def _fresh(name, like):
    """a freshly constructed module loaded with `like`'s state dict"""
    m = PACKS[name][0]()
    m.load_state_dict(like.state_dict())
    return m.eval()


@pytest.fixture(params=sorted(PACKS))
def case(request):
    name = request.param
    make, get, reads_bn = PACKS[name]
    m = _randomise(make(), 7)
    assert get(m) is not None, f"{name}: this module has no such pack"
    return name, m, get, reads_bn


def test_same_object_until_a_tensor_it_reads_changes(case):
    name, m, get, reads_bn = case
    first = get(m)
    assert get(m) is first
    for pname, p in m.named_parameters():
        before = get(m)
        assert get(m) is before
        with torch.no_grad():
            p.add_(1.0)
        after = get(m)
        assert after is not before, f"{name}: the old pack after {pname}.add_"
        assert _same(after, get(_fresh(name, m))), f"{name}: not the fresh module's pack after {pname}.add_"
    stats = [(n, b) for n, b in m.named_buffers() if n.endswith(("running_mean", "running_var"))]
    assert bool(stats) == reads_bn
    for bname, b in stats:
        before = get(m)
        with torch.no_grad():
            b.add_(1.0)
        after = get(m)
        assert after is not before, f"{name}: the old pack after {bname}.add_"
        assert not _same(after, before), f"{name}: {bname} is not folded in"
        assert _same(after, get(_fresh(name, m))), f"{name}: not the fresh module's pack after {bname}.add_"


def test_folded_pack_follows_the_final_convolution():
    dec, fc = _randomise(_decoder(), 3), _randomise(_final(), 4)
    before = dec.folded_pack(fc)
    assert dec.folded_pack(fc) is before
    with torch.no_grad():
        fc.weight.add_(1.0)
    after = dec.folded_pack(fc)
    assert after is not before and _same(after, _randomise(_decoder(), 3).folded_pack(fc))


def test_rebuilt_after_load_state_dict_and_after_a_dtype_round_trip(case):
    name, m, get, _ = case
    before = get(m)
    other = _randomise(PACKS[name][0](), 8)
    m.load_state_dict(other.state_dict())
    loaded = get(m)
    assert loaded is not before and _same(loaded, get(other)) and not _same(loaded, before)
    m.double().float()
    again = get(m)
    assert again is not loaded and _same(again, loaded)


def test_deepcopy_starts_empty_and_is_right(case):
    name, m, get, _ = case
    built = get(m)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)                                   # the original's cached pack is now stale; the copy must not carry it along
    twin = copy.deepcopy(m)
    for cache in [v for mod in twin.modules() for v in mod.__dict__.values() if type(v).__name__ == "ParamCache"]:
        assert cache._items == {}
    got = get(twin)
    assert got is not built and _same(got, get(_fresh(name, m))) and not _same(got, built)
    with torch.no_grad():
        for p in twin.parameters():                       # the copy follows its OWN tensors
            p.add_(1.0)
    assert get(twin) is not got and get(m) is get(m)
    assert not _same(get(twin), get(m))


def test_two_threads_get_one_object(case):
    name, m, get, _ = case
    m = _randomise(PACKS[name][0](), 9)                    # nothing built, no tensor list held yet
    got, gate = [None] * 8, threading.Barrier(8)

    def work(i):
        gate.wait()
        got[i] = get(m)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got[0] is not None and all(g is got[0] for g in got)


def test_assigning_a_parameter_or_buffer_starts_a_new_generation():
    lin = _randomise(HipLinear(6, 5), 1)
    before = lin.packed()
    lin.weight = torch.nn.Parameter(lin.weight.detach() + 1.0)         # a NEW tensor object at version 0
    after = lin.packed()
    assert after is not before and torch.equal(after[0][:, :6], lin.weight.detach())
    fc = _randomise(_final(), 2)
    g0 = generation(fc)
    assert generation(fc) == g0
    fc.register_buffer("extra", torch.zeros(1))
    fc.extra = torch.ones(1)
    assert generation(fc) != g0


def test_generation_names_device_versions_and_extra():
    stack = _randomise(MLP([4, 8, 8]), 5)
    g0 = generation(stack)
    assert generation(stack) == g0 and generation(stack, "lay") != g0 and generation(stack, "lay")[-1] == "lay"
    with torch.no_grad():
        stack[1][2].num_batches_tracked.add_(1)           # every buffer, recursively
    assert generation(stack) != g0
    only = [stack[0][0].weight]
    g1 = generation(stack, tensors=only)
    with torch.no_grad():
        stack[0][0].bias.add_(1.0)
    assert generation(stack, tensors=only) == g1
    with torch.no_grad():
        stack[0][0].weight.add_(1.0)
    assert generation(stack, tensors=only) != g1
    plain = torch.nn.Linear(3, 2)                         # any module: walked at every call, nothing held
    gp = generation(plain)
    assert generation(plain) == gp and "_held" not in plain.__dict__
    with torch.no_grad():
        plain.bias.add_(1.0)
    assert generation(plain) != gp


def test_batch_stats_packs_ignore_the_buffers_of_a_training_batchnorm():
    stack = _randomise(MLP([4, 8, 8]), 6)
    stack[0][2].train()                                   # block 0 normalises with the batch's statistics, block 1 stays in eval mode
    first = A._batch_stats_layers(stack)
    assert first[0][2] is None and first[0][3] is None and first[1][2] is not None
    with torch.no_grad():                                 # what every training forward does to block 0's buffers
        stack[0][2].running_mean.add_(1.0)
        stack[0][2].running_var.add_(1.0)
        stack[0][2].num_batches_tracked.add_(1)
    assert A._batch_stats_layers(stack) is first
    with torch.no_grad():
        stack[1][2].running_mean.add_(1.0)                # an eval-mode BatchNorm's statistics ARE read
    second = A._batch_stats_layers(stack)
    assert second is not first and not torch.equal(second[1][3], first[1][3])
    with torch.no_grad():
        stack[0][0].weight.add_(1.0)
    third = A._batch_stats_layers(stack)
    assert third is not second and torch.equal(third[0][0][:, :4], stack[0][0].weight.detach())
    stack[0][2].eval()                                    # the modes are part of the generation
    assert A._batch_stats_layers(stack) is not third


def test_transposed_pack_of_the_backward_keeps_its_cache_name_and_keys():
    lin = _randomise(HipLinear(6, 5), 2)

    class Ctx:
        owner, idx, k = lin, 0, 6
        wp = lin.packed()[0]
    wt = A._wt_pack(Ctx, lin.weight)
    assert set(param_cache(lin, "_grad_packs")._items) == {("wt", 0)} and A._wt_pack(Ctx, lin.weight) is wt
    assert torch.equal(wt[:, :5], lin.weight.detach().t())
    with torch.no_grad():
        lin.weight.add_(1.0)
    Ctx.wp = lin.packed()[0]
    assert A._wt_pack(Ctx, lin.weight) is not wt


def test_split_pack_keys_and_layout_in_the_generation():
    conv = _randomise(_conv(True), 3)
    a = conv.weight_pack("split", _LAY, mode=ops.SPLIT_F16X2)
    conv.weight_pack("wino", _LAY)
    conv.weight_pack("bwd_data_split", _LAY)
    assert set(param_cache(conv, "_split_packs")._items) == {"padded_weight", ops.SPLIT_F16X2, "wino", "bwd_data_split"}
    assert conv.weight_pack("split", _LAY, mode=ops.SPLIT_F16X2, device=True) is a            # (a CPU weight: the host builder, the host key)
    other = U._Layout(((24,), (32,), 64))                 # another layout: another generation of the same cache
    assert conv.weight_pack("padded_weight", other).shape[0] == 64
    assert set(param_cache(conv, "_split_packs")._items) == {"padded_weight"}
    assert conv._padded_weight(_LAY).shape[0] == 32


def test_fused_adam_still_accepts_a_module_and_the_modules_keywords():
    lin = HipLinear(6, 5)
    assert [id(p) for g in FusedAdam(lin).param_groups for p in g["params"]] == [id(p) for p in lin.parameters()]
    opt = FusedAdam(lin.parameters(), modules=lin)
    assert not hasattr(opt, "bind") and not hasattr(opt, "_owners")
    assert FusedAdam(lin.parameters(), modules=[lin, lin]).step(modules=lin) is None          # (no gradient yet: nothing is launched)
    assert opt.step(modules=[lin]) is None
