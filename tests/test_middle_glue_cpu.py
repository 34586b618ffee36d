"""The torch glue of the middle scan (porechop_amd/middle.py: TorchGlue) against the plain host reference, through the case
bodies the GPU holds the Aligner's kernels to (tests/glue_cases.py, tests/test_gpu_glue_kernels.py): one contract, two
implementations.  And the selecting step, which the GPU checks in a child process (tests/mask_rule_child.py), against the
header's rule as the library compiles it for the host."""
import numpy as np
import pytest
import torch

from tests import glue_cases
from tests.glue_cases import SIZES


@pytest.fixture(scope="module")
def glue():
    from porechop_amd.middle import TorchGlue
    return TorchGlue()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize("n", SIZES)
def test_trim_windows_equals_python_slices(glue, n):
    glue_cases.trim_windows_equal_python_slices(glue, dev, n)


def test_trim_windows_edges(glue):
    glue_cases.trim_windows_edges(glue, dev)


@pytest.mark.parametrize("n", SIZES)
def test_middle_hits_equal_the_reference(glue, n):
    glue_cases.middle_hits_equal_the_reference(glue, dev, n)


def test_middle_hits_keep_the_batch_shape_and_accept_an_empty_batch(glue):
    glue_cases.middle_hits_keep_the_batch_shape_and_accept_an_empty_batch(glue, dev)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("A", [1, 2, 7, 33])
def test_round_consume_equals_one_round_of_find_middle_adapters(glue, n, A):
    glue_cases.round_consume_equals_one_round_of_find_middle_adapters(glue, dev, n, A)


@pytest.mark.parametrize("n", SIZES + [0])
@pytest.mark.parametrize("words", [1, 3])
def test_group_survivors_equal_the_masked_any(glue, n, words):
    glue_cases.group_survivors_equal_the_masked_any(glue, dev, n, words)


@pytest.mark.parametrize("floored,nact,S", glue_cases.SELECT_CASES)
def test_round_consume_select_equals_the_headers_rule(glue, floored, nact, S):
    glue_cases.round_consume_select_equals_the_headers_rule(glue, dev, floored, nact, S)


def test_the_glue_of_a_call_follows_the_aligner_and_the_switch(monkeypatch):
    """choose_glue: an aligner without the native steps gets the torch glue; one with them is its own glue unless
    PC_NO_FUSED_GLUE is set, which is read per call; copy_windows goes to the aligner's wherever it has one."""
    from porechop_amd.middle import GLUE_STEPS, TorchGlue, choose_glue

    class Bare:
        pass

    class Native:
        STAT_BIG = TorchGlue.STAT_BIG

        def copy_windows(self, *a):
            return "native copy"
    for step in GLUE_STEPS:
        setattr(Native, step, lambda self, *a: None)
    monkeypatch.delenv("PC_NO_FUSED_GLUE", raising=False)
    bare, native = Bare(), Native()
    assert isinstance(choose_glue(bare), TorchGlue)
    assert choose_glue(bare).copy_windows.__func__ is TorchGlue.copy_windows
    assert choose_glue(native) is native
    monkeypatch.setenv("PC_NO_FUSED_GLUE", "0")
    assert choose_glue(native) is native
    monkeypatch.setenv("PC_NO_FUSED_GLUE", "1")
    glue = choose_glue(native)
    assert isinstance(glue, TorchGlue) and glue.copy_windows() == "native copy"
