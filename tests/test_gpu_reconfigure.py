"""Reconfiguring a live problem equals building a fresh one, on the GPU: the walks of reconfigure_walks.py (the same tables
test_cpu_reconfigure.py runs on the CPU build), with the switches that only mean something here -- "mfma_stiffness" at
N = 11, "amg_graph" with a stream that can be captured, the hierarchy built with "amg_device_setup", the 32-bit V-cycle and
inner solve on the device.  Every step of a walked problem gives the bits of a fresh problem at that configuration; the
last step of one walk per family is also held to the oracle (1e-9, as test_gpu_host.py does).

The host layer runs on a stream of its own (as in test_gpu_amg.py) so that the V-cycle is captured and replayed: a graph
that outlives the setting it was captured under is one of the things a walk must see."""
import pytest

import reconfigure_walks as R
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own_stream(gpu):
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    yield True
    H.init(0)  # back to torch's current stream for the other modules


@pytest.mark.parametrize("walk", R.walk_names(cpu=False))
def test_reconfigured_problem_equals_a_fresh_one(own_stream, walk):
    R.run_walk(R.Driver(H, S, lib), walk)


@pytest.mark.parametrize("name", sorted(R.ABANDONED))
def test_an_abandoned_stepwise_run_leaves_nothing_behind(own_stream, name):
    R.run_abandoned_stepwise(R.Driver(H, S, lib), name)


def test_the_device_built_hierarchy_is_walked_here():
    assert "vcycle_device" in R.walk_names(cpu=False) and R.WALKS["vcycle_device"]["base"]["amg"] == "device"
