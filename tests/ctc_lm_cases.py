"""Models and configurations of the LM-fused prefix beam search tests (tests/test_ctc_lm_restatement.py on the CPU,
tests/test_gpu_ctc_decode_lm.py on the GPU).  The minibatches are tests/ctc_decode_cases.py's; the models come from
tests/ctc_lm_restatement.py: random_model with the seeds recorded here.

A seed is part of the case: the CPU test holds the stability cap (at most S // 8 unstable utterances) on exactly these, and a seed
that misses it is replaced here, never the cap."""

# name -> arguments of random_model
MODELS = {
    "k2_o2": dict(seed=4101, K=2, order=2, named=False),
    "k7_o1": dict(seed=4102, K=7, order=1, named=False),
    "k7_o2": dict(seed=4103, K=7, order=2, named=True),
    "k7_o4_unk": dict(seed=4104, K=7, order=4, missing=(5,), unk=True, named=True),
    "k46_o3": dict(seed=4105, K=46, order=3, named=True),
    "k40_o3": dict(seed=4106, K=40, order=3, named=False),
    "k30_o4": dict(seed=4107, K=30, order=4, named=True),
    "k100_o3": dict(seed=4108, K=100, order=3, named=False),
    "k3_o3": dict(seed=4109, K=3, order=3, named=True),            # exhaustive
    "k5_o3": dict(seed=4110, K=5, order=3, named=False),           # uniform
    "k12_o3_noeos": dict(seed=4111, K=12, order=3, eos=False, bos=False, named=False),   # ties; no <s>, no </s>
}

# key -> the minibatch, (beam, max_classes), the model and the fusion parameters
CASES = {
    "k2": dict(case="k2", B=8, C=1, model="k2_o2", alpha=0.7, beta=0.3, eos=True),
    "dense_3x12x7_1x6": dict(case="dense_3x12x7", B=1, C=6, model="k7_o1", alpha=0.9, beta=-0.5, eos=False),
    "dense_3x12x7_3x1": dict(case="dense_3x12x7", B=3, C=1, model="k7_o2", alpha=0.5, beta=1.0, eos=True),
    "dense_3x12x7_16x6": dict(case="dense_3x12x7", B=16, C=6, model="k7_o4_unk", alpha=0.8, beta=0.2, eos=True),
    "dense_8x60x46": dict(case="dense_8x60x46", B=16, C=20, model="k46_o3", alpha=0.6, beta=0.4, eos=True),
    "peaky_h4_60": dict(case="peaky_h4_60", B=16, C=20, model="k40_o3", alpha=1.0, beta=-0.2, eos=False),
    "peaky_T1500": dict(case="peaky_T1500", B=4, C=4, model="k30_o4", alpha=0.75, beta=0.1, eos=True),
    "dense_33x40x100": dict(case="dense_33x40x100", B=32, C=64, model="k100_o3", alpha=0.5, beta=0.6, eos=True),
}
EXHAUSTIVE = dict(case="exhaustive", B=64, C=2, model="k3_o3", alpha=0.8, beta=0.5, eos=True)
TIE_MODELS = {"ties": "k12_o3_noeos", "uniform": "k5_o3"}

# The two models of about 10^5 n-grams behind the timing rows of profiles/ctc_decode_lm.md (arguments of random_model; K = 46, the
# posterior shape of profiles/ctc_decode.md: tests/ctc_cases.peaky_case(32, 1000, 46, 100, (4, 12, 30), 101)).  No test builds them.
TIMING_MODELS = {
    "k46_o3_dense": dict(seed=4201, K=46, order=3, fill=0.95, per_order={2: 100000, 3: 100000}),            # 87 972 n-grams
    "k46_o5_sparse": dict(seed=4202, K=46, order=5, per_order={2: 1400, 3: 20000, 4: 40000, 5: 40000}),     # 101 448 n-grams
}
