"""CPU side of the batched external evaluator (az_set_external_evaluator): the header declares the entry points and the
library exports them, a NULL engine is refused without a crash, the Python wrappers check their arguments before they touch
the library, and MCTS dispatches on controller.BatchPolicyValueFn.  What runs on the GPU is in test_external_eval_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

import alphazero_piskvorky_amd as az
from alphazero_piskvorky_amd import _capi, net
from alphazero_piskvorky_amd.controller import (BatchPolicyValueFn, PolicyValueFn, make_batch_policy_value_fn,
                                                merge_batch_evaluators)
from alphazero_piskvorky_amd.evaluator import ModelEvaluator
from alphazero_piskvorky_amd.mcts import MCTS
from alphazero_piskvorky_amd.self_play import SelfPlayManager
from tests.util import ROOT

SYMBOLS = ["az_set_external_evaluator", "az_get_external_evaluator", "az_ext_capacity", "az_ext_stats"]


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    declared = set(re.findall(r"\b(az_[a-z_0-9]+)\s*\(", hdr))
    L = ctypes.CDLL(_capi.LIB_PATH)
    for s in SYMBOLS:
        assert s in declared, f"{s} is not declared in include/az_engine.h"
        assert hasattr(L, s), f"{s} is not exported by the library"
        assert s in _capi.EXPORTS
    assert "az_eval_batch_fn" in hdr and "az_ext_evaluator" in hdr
    # the struct of the binding has the header's fields, in its order
    assert [f for f, _ in _capi.az_ext_evaluator._fields_] == ["planes_dev", "policy_dev", "value_dev", "capacity", "fn", "user"]
    body = re.search(r"typedef struct \{([^}]*)\} az_ext_evaluator;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == ["planes_dev", "policy_dev", "value_dev", "capacity", "fn", "user"]


def test_a_null_engine_is_refused_without_a_crash():
    L = _capi.lib()
    cb = _capi._EVAL_BATCH_FN(lambda user, net_id, count: 0)
    ev = _capi.az_ext_evaluator(16, 16, 16, 4, cb, None)
    assert L.az_set_external_evaluator(None, ctypes.byref(ev)) == -1
    assert L.az_set_external_evaluator(None, None) == -1
    assert L.az_get_external_evaluator(None) == -1
    assert L.az_ext_capacity(None) == -1
    r, i = ctypes.c_int64(5), ctypes.c_int64(6)
    assert L.az_ext_stats(None, ctypes.byref(r), ctypes.byref(i)) == -1
    assert (r.value, i.value) == (5, 6)


def test_the_wrapper_checks_its_arguments_before_the_library():
    e = az.Engine.__new__(az.Engine)         # no GPU here: the checks below come before any call into the library
    e.h, e._ext_err, e._ext_cb = ctypes.c_void_p(), [], None
    with pytest.raises(TypeError):
        e.set_external_evaluator(16, 16, 16, 4, None)
    for ptrs in ((0, 16, 16), (16, 0, 16), (16, 16, None)):
        with pytest.raises(ValueError):
            e.set_external_evaluator(*ptrs, 4, lambda net_id, count: None)
    with pytest.raises(ValueError):
        e.set_external_evaluator(16, 16, 16, 0, lambda net_id, count: None)
    with pytest.raises(TypeError):
        BatchPolicyValueFn(None)
    with pytest.raises(TypeError):
        make_batch_policy_value_fn(lambda planes: planes)
    with pytest.raises(TypeError):
        make_batch_policy_value_fn((net.GomokuNet(board_size=5),) * 3)
    with pytest.raises(TypeError):
        merge_batch_evaluators((1, 2))
    with pytest.raises(TypeError):
        SelfPlayManager(None, "cuda:0", evaluator=lambda planes, net_id: None)
    with pytest.raises(ValueError):
        SelfPlayManager(None, "cuda:0", evaluator=BatchPolicyValueFn(lambda planes, net_id: None), leaf_symmetry=True)
    with pytest.raises(TypeError):
        ModelEvaluator(device="cuda:0", evaluators=(lambda planes, net_id: None,) * 2)
    assert ModelEvaluator(device="cuda:0", evaluators=True).evaluators is True


def test_mcts_dispatches_on_the_evaluator_kind():
    batched = MCTS(BatchPolicyValueFn(lambda planes, net_id: None), num_simulations=8, c_puct=2.0)
    assert batched._batched and not batched._external
    plain = MCTS(lambda state: None, num_simulations=8, c_puct=2.0)
    assert plain._external and not plain._batched
    native = MCTS(PolicyValueFn(None), num_simulations=8, c_puct=2.0)
    assert not native._external and not native._batched
    with pytest.raises(TypeError):
        MCTS(None, num_simulations=8, c_puct=2.0)


def test_make_batch_policy_value_fn_keeps_the_forward_contract():
    n = 5
    torch.manual_seed(0)
    m = net.GomokuNet(board_size=n).eval()
    bf = make_batch_policy_value_fn(m)
    planes = (torch.rand(7, 4, n, n) < 0.3).float()
    P, v = bf.fn(planes, 0)
    assert P.shape == (7, n * n) and v.reshape(-1).shape == (7,) and not P.requires_grad
    assert torch.allclose(P.sum(dim=1), torch.ones(7), atol=1e-5) and bool((P >= 0).all())
    logits, value = m(planes)
    # the module sees the request padded to 16 rows: the same numbers within the tolerances torch is granted here
    assert torch.allclose(P, torch.softmax(logits.detach(), dim=1), rtol=0, atol=1e-6)
    assert torch.allclose(v, value.detach(), rtol=0, atol=2e-6)
    other = net.GomokuNet(board_size=n).eval()
    pair = make_batch_policy_value_fn((m, other))
    assert torch.equal(pair.fn(planes, 0)[0], P) and not torch.allclose(pair.fn(planes, 1)[0], P, rtol=0, atol=1e-4)
    merged = merge_batch_evaluators((bf, make_batch_policy_value_fn(other)))
    assert torch.equal(merged.fn(planes, 1)[0], pair.fn(planes, 1)[0])
    # a request of another size reuses or adds a scratch batch; rows behind the request do not leak into its results
    P3, _ = bf.fn(planes[:3], 0)
    assert P3.shape == (3, n * n) and torch.allclose(P3, P[:3], rtol=0, atol=1e-6)
