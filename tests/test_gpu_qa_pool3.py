"""mn_qa_* with pool = 2 (csrc/qact_pool3.h) on the MI355X: the case table of tests/qa_pool3_cases.py."""
import pytest

import abi_driver
import qa_pool3_cases as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("shape, kind, bits, quant, training", Q.CASES, ids=Q.IDS)
def test_qa_pool3(be, shape, kind, bits, quant, training):
    Q.check(be, shape, kind, bits, quant, training)


def test_qa_pool3_refused(be):
    Q.check_refused(be)
