"""The sparse-training Adam step (k_adam_l1: the L1 sub-gradient of channel pruning inside the one-launch optimizer step) on the CPU SIMT emulator, against
torch.optim.Adam + the reference's updateBN() (tests/prune_cases.py).  The same checks run on the MI355X in test_gpu_prune.py."""
import pytest

import abi_driver
import prune_cases as P


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


def test_adam_l1_matches_torch_with_updatebn(be):
    P.check_adam_l1(be)


def test_adam_l1_more_tensors_than_one_table(be):
    P.check_adam_l1_many(be)


def test_adam_l1_zero_is_the_plain_step_bit_for_bit(be):
    P.check_l1_zero_is_plain(be)


def test_adam_l1_rejects_bad_arguments(be):
    P.check_l1_rejects_bad_arguments(be)
