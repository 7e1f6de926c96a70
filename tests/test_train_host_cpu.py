"""Host-side helpers of the training path that need no GPU."""
import pytest
import torch

from uni_renderer_amd import param_stage as PS
from uni_renderer_amd import train_step as TS
from uni_renderer_amd.controlnet import CIN_PAD


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(8, 8)
        self.c1 = torch.nn.Conv2d(8, 8, 1)
        self.c3 = torch.nn.Conv2d(8, 8, 3, padding=1)
        self.norm = torch.nn.LayerNorm(8)


def test_parameter_list_is_cached_per_network_tuple():
    nets = (_Net(), _Net(), _Net())
    ps = TS._parameters(nets)
    assert len(ps) == sum(1 for n in nets for _ in n.parameters())
    assert TS._parameters(nets) is ps                      # same tuple of networks: the cached list
    other = (_Net(), nets[1], nets[2])
    assert TS._parameters(other) is not ps and TS._parameters(other)[0] is other[0].lin.weight


def _staged(stage):
    return (stage.weights, stage.merged, stage.vectors, stage.packed)


def test_batched_casts_cover_linear_and_1x1_weights_and_fail_loudly_on_cpu():
    net = _Net()
    with torch.no_grad():                                  # inference: nothing is staged up front
        with PS.Stage(net, torch.bfloat16) as st:
            assert PS.active is st and not any(_staged(st))
    assert PS.active is None
    with pytest.raises(RuntimeError):                      # training on CPU tensors: no CPU fallback
        with PS.Stage(net, torch.bfloat16):
            pass
    ws = PS.plan(net).matrices
    assert {id(w) for w in ws} == {id(net.lin.weight), id(net.c1.weight)}  # Linear + 1x1 conv; not the 3x3, not the norm
    assert PS.active is None                               # after leaving, by the exception too: nothing is staged
    w = PS.wc(net.lin.weight, torch.bfloat16)              # outside a stage: the plain differentiable cast
    assert w.dtype == torch.bfloat16 and w.requires_grad


def test_a_dropped_network_takes_its_stage_plan_along():
    import gc

    net = _Net()
    assert PS.plan(net) is PS.plan(net) and net in PS._plans
    del net
    gc.collect()
    assert len(PS._plans) == 0


def test_a_stage_left_by_an_exception_leaves_nothing_to_the_next_one():
    a, b = _Net(), _Net()
    with torch.no_grad():
        with pytest.raises(KeyError):
            with PS.Stage(a, torch.bfloat16) as st:
                st.weights[id(a.lin.weight)] = a.lin.weight.to(torch.bfloat16)   # as if staged
                st.vectors[id(a.lin.bias)] = a.lin.bias
                assert PS.wc(a.lin.weight, torch.bfloat16) is st.weights[id(a.lin.weight)]
                raise KeyError("in the body")
        assert PS.active is None
        with PS.Stage(b, torch.bfloat16) as st2:
            assert PS.active is st2 and not any(_staged(st2))
            assert PS.wc(a.lin.weight, torch.bfloat16) is not st.weights[id(a.lin.weight)]
        with pytest.raises(RuntimeError):                  # the networks run one after the other: no stage inside a stage
            with PS.Stage(a, torch.bfloat16):
                with PS.Stage(b, torch.bfloat16):
                    pass
    assert PS.active is None


def test_stage_plan_order_keeps_concatenated_operands_adjacent_and_leaves_the_narrow_convs_out():
    """The packed copies lie in plan order and ``cat_adjacent`` relies on it: all time_emb_proj, then the to_k / to_v pairs of
    the cross-attentions, then the rest in module order.  The seven narrow convs of a ControlNet conditioning embedding are
    neither packed nor put behind the bias barrier (CondConv3x3 reads the parameters themselves); its conv_out is an ordinary
    3x3 conv."""
    from uni_renderer_amd.layers import BasicTransformerBlock, ControlNetConditioningEmbedding, ResnetBlock2D

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv_in = torch.nn.Conv2d(4, 32, 3, padding=1)
            self.r0 = ResnetBlock2D(32, 32, 128, groups=8)
            self.tb = BasicTransformerBlock(32, 2, 16, 64)
            self.r1 = ResnetBlock2D(64, 32, 128, groups=8)           # with a 1x1 shortcut
            self.controlnet_cond_embedding = ControlNetConditioningEmbedding(32, 3, (16, 32))

    net = Toy()
    p = PS.plan(net)
    tb, emb = net.tb, net.controlnet_cond_embedding
    rest = [tb.attn1.to_q.weight, tb.attn1.to_k.weight, tb.attn1.to_v.weight, tb.attn1.to_out[0].weight, tb.attn2.to_q.weight,
            tb.attn2.to_out[0].weight, tb.ff.net[0].proj.weight, tb.ff.net[2].weight, net.r1.conv_shortcut.weight]
    want = [net.r0.time_emb_proj.weight, net.r1.time_emb_proj.weight, tb.attn2.to_k.weight, tb.attn2.to_v.weight] + rest
    assert [id(w) for w in p.matrices] == [id(w) for w in want]
    narrow = [emb.conv_in] + list(emb.blocks)
    assert len(narrow) == 3 and all(m.kernel_size == (3, 3) for m in narrow)
    vec, c3 = {id(v) for v in p.vectors}, {id(w): cp for w, cp in p.convs}
    assert not any(id(m.bias) in vec or id(m.weight) in c3 for m in narrow)
    assert id(emb.conv_out.bias) in vec and c3[id(emb.conv_out.weight)] is None
    assert c3[id(net.conv_in.weight)] == CIN_PAD and id(net.r0.norm1.weight) in vec and id(tb.norm3.bias) in vec
    assert [id(w) for w, _ in p.convs] == [id(m.weight) for m in (net.conv_in, net.r0.conv1, net.r0.conv2, net.r1.conv1,
                                                                   net.r1.conv2, emb.conv_out)]


def test_derived_weight_cache_never_serves_a_dead_buffer():
    """the W^T / rotated-weight caches are keyed by raw address; an entry must die with the buffer it was derived
    from (a later tensor at the same address with the same shape would otherwise pick up a stale transpose)."""
    import gc

    import torch

    from uni_renderer_amd.backward import _DerivedWeights

    cache = _DerivedWeights()
    owner = torch.zeros(4, 4)
    key = (owner.data_ptr(), (4, 4))
    cache.put(key, owner, torch.ones(4, 4))
    assert torch.equal(cache.lookup(key), torch.ones(4, 4))
    del owner
    gc.collect()
    assert cache.lookup(key) is None and key not in cache  # the dead entry is a miss and is dropped
    o2 = torch.zeros(2, 2)
    cache.put((1, (2, 2)), o2, torch.ones(2, 2))
    o3 = torch.zeros(3)
    cache.put((2, (3,)), o3, torch.ones(3))
    del o3
    gc.collect()
    cache.sweep()
    assert list(cache) == [(1, (2, 2))]


def test_norm_sums_defer_each_parameter_once_and_never_under_anomaly_detection():
    """a norm layer (or tied gamma / beta) used twice before a flush must not hand out two uninitialised results
    that autograd adds at once; anomaly detection inspects node outputs immediately."""
    import torch

    from uni_renderer_amd.backward import NormSums

    ns = NormSums()
    g1, g2 = torch.ones(8), torch.ones(8)
    assert ns.fresh(g1) and ns.fresh(g2)
    assert not ns.fresh(g1)  # the repeat takes the immediate path
    ns.reset()
    assert ns.fresh(g1)
    ns.reset()
    with torch.autograd.detect_anomaly(check_nan=False):
        assert not ns.fresh(g1)


def test_grad_sink_first_writer_stores_later_writers_add():
    """Round 6: gradients living in communication buckets are WRITTEN there by the kernels that produce them
    (backward.GradSink) instead of being added into zeroed buckets by autograd.  Host logic: the first ``take`` of a parameter
    since ``begin`` hands out the destination, later ones (second pass of the cycle branch, accumulation micro-steps) get None
    = the ordinary add path; anomaly mode and ``end()`` switch the sink off."""
    import torch
    from uni_renderer_amd import backward as B

    store = {1: torch.zeros(3), 2: torch.zeros(2)}
    sink = B.GradSink()
    assert sink.take(1) is None  # no provider installed
    sink.begin(lambda pid: store.get(pid))
    assert sink.take(1) is store[1] and sink.take(1) is None and sink.take(3) is None and sink.take(2) is store[2]
    sink.begin(lambda pid: store.get(pid))  # next optimisation step
    with torch.autograd.detect_anomaly(check_nan=False):
        assert sink.take(1) is None
    assert sink.take(1) is store[1]
    sink.end()
    assert sink.take(2) is None
    # cast_many(outs=...) validates its destinations before touching the device
    import pytest
    with pytest.raises(ValueError):
        B.cast_many([torch.zeros(4, dtype=torch.bfloat16)], torch.float32, outs=[torch.zeros(3)])
