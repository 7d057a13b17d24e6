"""GPU: the device instantiation of csrc/pairing_tower.hpp, one lane per case (zkp_selftest_fq12_dev, zkp_selftest_miller_dev), against
the big-int model of the same algorithms (tests/model/pairing_fast_model.py), bit for bit: every operation at coefficients 0, 1 and
p - 1 in every slot plus random ones -- 65 cases, so that a second wave with one live lane runs -- then the Miller value of one pair
against the plain model's miller_loop, E of it against the plain model's pairing cubed, and the value a k = 2 check returns against
the product of the two model pairings, cubed."""
import numpy as np
import pytest

import bigmodel as M
import pairing_cases as PC
import pairing_fast_model as FM
import pairing_model as PM

pytestmark = pytest.mark.gpu
N_CASES = 65


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def pairing_module():
    import zkp_hip.pairing
    return zkp_hip.pairing


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


def f12_array(elems):
    return np.array([FM.f12_to_words(e) for e in elems], dtype=np.uint64)


def g2_limbs(q):
    return np.array([w for f2 in q for c in f2 for w in M.to_limbs(M.fq_to_mont(c), 6)], dtype=np.uint64)


def g1_limbs(p):
    return np.array([w for c in p for w in M.to_limbs(M.fq_to_mont(c), 6)], dtype=np.uint64)


@pytest.fixture(scope="module")
def operands():
    a = PC.edge_elements() + PC.random_elements(0xA11CE, N_CASES - 6)
    b = PC.random_elements(0xB0B, N_CASES - 6) + PC.edge_elements()
    return a, b


@pytest.mark.parametrize("op", list(PC.OPS))
def test_fq12_operation_bit_for_bit(zkp, operands, op):
    import torch
    number, two, model = PC.OPS[op]
    a, b = operands
    want = f12_array([model(x, y) for x, y in zip(a, b)])
    out = torch.zeros(N_CASES * 72, dtype=torch.int64, device="cuda")
    pairing_module().selftest_fq12_dev(number, dev(f12_array(a)), dev(f12_array(b)) if two else None, N_CASES, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64).reshape(N_CASES, 72)
    bad = [i for i in range(N_CASES) if not np.array_equal(got[i], want[i])]
    assert not bad, (op, bad[:8])


def test_fq12_selftest_refusals(zkp):
    import torch
    pm = pairing_module()
    t = torch.zeros(72, dtype=torch.int64, device="cuda")
    o = torch.zeros(72, dtype=torch.int64, device="cuda")
    for call in (lambda: pm.selftest_fq12_dev(9, t, t, 1, o), lambda: pm.selftest_fq12_dev(-1, t, t, 1, o), lambda: pm.selftest_fq12_dev(1, t, None, 1, t)):
        with pytest.raises(zkp.ZkpError) as ei:
            call()
        assert ei.value.code == zkp.ZKP_E_ARG


def test_miller_value_and_final_exponentiation_against_the_plain_model(zkp):
    import torch
    pm = pairing_module()
    p2, q2 = M.g1_mul(M.G1, 0xC0FFEE), PM.g2_mul(PM.G2, 0xBEEF)
    one = pm.PairingChecker(g2_limbs(PM.G2).reshape(1, 24), 4)
    out = torch.zeros(72, dtype=torch.int64, device="cuda")
    one.miller_dev(dev(g1_limbs(M.G1)), 1, out)
    torch.cuda.synchronize()
    miller = PM.miller_loop(M.G1, PM.G2)
    assert out.cpu().numpy().view(np.uint64).tolist() == FM.f12_to_words(miller)
    pairing_g = PM.f12_pow(miller, PM.FINAL_EXP)                     # = PM.pairing(G1, G2)
    ok, val = one.check_batch(g1_limbs(M.G1).reshape(1, 1, 12), values=True)
    assert ok.tolist() == [0]
    assert val.reshape(72).tolist() == FM.f12_to_words(PM.f12_pow(pairing_g, 3))
    two = pm.PairingChecker(np.stack([g2_limbs(PM.G2), g2_limbs(q2)]), 4)
    ok, val = two.check_batch(np.stack([g1_limbs(M.G1), g1_limbs(p2)]).reshape(1, 2, 12), values=True)
    product = PM.f12_mul(pairing_g, PM.pairing(p2, q2))
    assert ok.tolist() == [0]
    assert val.reshape(72).tolist() == FM.f12_to_words(PM.f12_pow(product, 3))
    assert val.reshape(72).tolist() == FM.f12_to_words(PM.f12_pow(pairing_g, 3 * (1 + 0xC0FFEE * 0xBEEF)))   # bilinear
