"""CPU: what tests/test_gpu_ctc_decode_lm.py relies on, held with the restatement alone (tests/ctc_lm_restatement.py).

  the fused restatement against enumeration: on `exhaustive` (K = 3, nothing is pruned at beam 64) with an order-3 model, alpha = 0.8,
      beta = 0.5 and eos, every labelling comes back with enumerate_paths' ln p + alpha * lm64 + beta * len
  over-counting: score <= lnp64(hyp) + alpha * lm64(hyp) + beta * len + bar for every entry of every case
  the stability cap: at most S // 8 utterances per case whose 1-best moves under the eight jitter seeds -- a condition on the cases
      (tests/ctc_lm_cases.py records the seeds), not a measurement
  fp32: the restatement run in float32 is within the bar of the fp64 one on the stable utterances, 1-best equal

The bar: bar_of(score64, n) of tests/ctc_beam_restatement.py on the fused score, plus |alpha| * (len + order + 1) * 2^-23 * sum|terms|
for the LM sum (each of its len + order fp32 additions rounds to 2^-24 of a partial sum that sum|terms| bounds; a factor 2 for the
fp32 storage of the weights).
"""
import numpy as np
import pytest

from tests import ctc_beam_restatement as R
from tests import ctc_decode_cases as dc
from tests import ctc_lm_cases as lc
from tests import ctc_lm_restatement as L


def test_fused_restatement_is_the_enumeration():
    cfg = lc.EXHAUSTIVE
    model = L.model_of(cfg["model"])
    assert model.order == 3 and (cfg["alpha"], cfg["beta"], cfg["eos"]) == (0.8, 0.5, True)
    lens, probs, T, S = dc.build(cfg["case"])
    for s in range(S):
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        got = L.beam_search(lp, R.log32(R.utterance(probs, s, S, n)), cfg["B"], cfg["C"], model, cfg["alpha"], cfg["beta"], True)
        want = {h: v + cfg["alpha"] * model.lm64(h, True)[0] + cfg["beta"] * len(h) for h, v in R.enumerate_paths(lp).items()}
        assert {h for h, _, _ in got} == set(want)
        for h, score, lmsum in got:
            assert abs(score - want[h]) <= 1e-12 * max(1.0, abs(want[h])), (s, h)
            assert abs(lmsum - model.lm64(h, True)[0]) <= 1e-12 * max(1.0, abs(lmsum)), (s, h)
        assert [h for h, _, _ in got] == sorted(want, key=want.get, reverse=True)


@pytest.mark.parametrize("key", list(lc.CASES))
def test_cases_hold_their_conditions(key):
    lens, probs, T, S, model, cfg, ref = L.case(key)
    alpha, beta, eos = cfg["alpha"], cfg["beta"], cfg["eos"]
    unstable = [s for s in range(S) if not ref[s]["stable"]]
    assert len(unstable) <= S // 8, (key, unstable)
    worst, changed = 0.0, 0
    plain = R.case(cfg["case"], cfg["B"], cfg["C"])[4]
    for s in range(S):
        r = ref[s]
        n = int(lens[s])
        lp = R.log64(R.utterance(probs, s, S, n))
        for h, score, lmsum in r["beam64"]:
            lm64, absum = model.lm64(h, eos)
            exact = R.lnp64(lp, h) + alpha * lm64 + beta * len(h)
            assert score <= exact + r["bar"], (key, s, h, score, exact)
            assert abs(lmsum - lm64) <= 1e-12 * max(1.0, absum), (key, s, h)
        changed += r["beam64"][0][0] != plain[s]["beam64"][0][0]
        if not r["stable"]:
            continue
        assert r["beam32"][0][0] == r["beam64"][0][0], (key, s)
        err = abs(r["beam32"][0][1] - r["score64"])
        assert err <= r["bar"], (key, s, err, r["bar"])
        lm_err = abs(r["beam32"][0][2] - r["beam64"][0][2])
        assert lm_err <= L.lm_term(model, alpha, r["beam64"][0][0], eos)[1], (key, s)
        worst = max(worst, err / r["bar"])
    print(f"{key}: unstable {unstable} (cap {S // 8}); fp32 |score - score64| / bar <= {worst:.3g}; the LM changed the 1-best on {changed}/{S}")
