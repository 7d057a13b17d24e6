"""GPU: the polled waits' opt-outs (csrc/knobs.hpp, poll_or_sync in csrc/dev_res.hpp) are honoured on every call, in both
directions, within one process: nothing about them is frozen at the first MSM or the first proof."""
import numpy as np
import pytest

import bigmodel as M
import plonk_model as PM
from test_plonk_model import challenges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available()
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def test_msm_result_wait_polled_or_not_call_by_call(zkp, orc, monkeypatch):
    """An unexpanded 3000-term MSM with ZKP_MSM_NO_POLL set, unset and set again: the oracle's inner-product point each time."""
    import torch
    n = 3000
    ks = orc.rand_fr(0x9011, n)
    sc = orc.rand_fr(0x9012, n)
    t_pts = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    zkp.g1_fixed_base_mul_dev(torch.from_numpy(ks.view(np.int64)).cuda(), n, t_pts)
    bases = zkp.G1Bases.from_device(t_pts, n)
    exp, einf = orc.g1_mul(orc.g1_generator(), 0, orc.fr_inner_product(sc, ks))
    for no_poll in (True, False, True):
        if no_poll:
            monkeypatch.setenv("ZKP_MSM_NO_POLL", "1")
        else:
            monkeypatch.delenv("ZKP_MSM_NO_POLL", raising=False)
        out, inf = zkp.msm_g1(bases, sc)
        assert inf == einf and np.array_equal(out, exp), f"ZKP_MSM_NO_POLL {'set' if no_poll else 'unset'}"


def test_plonk_read_back_wait_polled_or_not_call_by_call(zkp, orc, monkeypatch):
    """One proof of the two-gate circuit (plonk/src/verifier.rs:361-383) per setting of ZKP_PLONK_NO_POLL -- unset, set, unset, set --
    from one prover: every proof equals the first."""
    cc = PM.reference_test_circuit_03().compile()
    blinders, _ = challenges(11)
    n = cc["n"]
    srs = zkp.Srs.new_from_secret(orc.fr_from_ints([M.rand_fr_list(0x9013, 1)[0]])[0], n)
    polys = {k: orc.fr_from_ints(cc[k]) if len(cc[k]) else np.zeros((0, 4), dtype=np.uint64) for k in zkp.CIRCUIT_POLYS}
    pr = zkp.PlonkProver(srs.bases, n.bit_length() - 1, polys, orc.fr_from_ints([cc["k1"]])[0], orc.fr_from_ints([cc["k2"]])[0])

    def flat(proof):
        commits = sorted(proof["commits"].items())
        return ([name for name, _ in commits], [np.asarray(xy).tobytes() for _, (xy, _) in commits], [bool(inf) for _, (_, inf) in commits],
                np.asarray(proof["bars"]).tobytes(), np.asarray(proof["u"]).tobytes(), int(proof["degree"]))

    monkeypatch.delenv("ZKP_PLONK_NO_POLL", raising=False)
    first = flat(pr.prove(orc.fr_from_ints(blinders)))
    assert len(first[0]) == 9
    for no_poll in (True, False, True):
        if no_poll:
            monkeypatch.setenv("ZKP_PLONK_NO_POLL", "1")
        else:
            monkeypatch.delenv("ZKP_PLONK_NO_POLL", raising=False)
        assert flat(pr.prove(orc.fr_from_ints(blinders))) == first, f"ZKP_PLONK_NO_POLL {'set' if no_poll else 'unset'}"
    pr.close()
