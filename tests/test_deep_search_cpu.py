"""Deep searches (az_create_deep, more than 1024 simulations per move): what can be checked without a GPU -- the C-ABI
declares the entry point, argument validation runs before the device is looked for, and the oracle that judges the
engine at deep S keeps the reference's visit arithmetic at any S."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests.util import ROOT

import alphazero_piskvorky_amd as az


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available() and torch.cuda.device_count() > 0
    except Exception:
        return False


def test_header_declares_the_deep_entry_point():
    with open(os.path.join(ROOT, "include", "az_engine.h")) as f:
        h = f.read()
    assert "int az_create_deep(const az_config *cfg, az_engine **out);" in h
    assert "#define AZ_DEEP_MAX_SIMULATIONS 65534" in h
    assert "az_create_deep" in az._capi.EXPORTS
    assert az._capi.AZ_DEEP_MAX_SIMULATIONS == 65534


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_deep_engine_passes_validation_then_needs_a_device():
    with pytest.raises(az.AzError, match="no HIP device"):
        az.Engine(5, 4, 10_000, 4, deep=True)


@pytest.mark.parametrize("S", [65_535, 0])
def test_deep_engine_rejects_out_of_range_simulations(S):
    with pytest.raises(az.AzError, match=r"\(-1\): num_simulations must be 1\.\.65534"):
        az.Engine(5, 4, S, 4, deep=True)


def test_default_engine_keeps_its_cap():
    with pytest.raises(az.AzError, match=r"\(-1\): num_simulations must be 1\.\.1024"):
        az.Engine(5, 4, 2000, 4)


@pytest.mark.parametrize("vl", [0, 8])
def test_oracle_search_at_deep_S_makes_every_simulation(vl):
    n, k, S = 5, 4, 4096
    o = orc.Oracle(n, k, S, synthetic=True, virtual_loss=vl)
    rs = np.random.RandomState(5)
    board = np.zeros(n * n, np.uint8)
    r = o.search(None, board, 1, -1, 1.0, rs.dirichlet([0.3] * (n * n)), 0.4)
    assert int(r["N"].sum()) == S
    assert int(r["N"].max()) > 2047          # beyond the default kernels' 11-bit visit field
