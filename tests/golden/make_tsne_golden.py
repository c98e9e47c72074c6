"""Writes tests/golden/g8_tsne.npz: the fixture of the t-SNE tests (tests/test_tsne_host.py, tests/test_gpu_tsne.py).

    X [384, 128] fp32   six Gaussian clusters of 64 points; labels [384]; Y0 [384, 2] fp32, scikit-learn's random start
    kl_sklearn          final KL of TSNE(method='exact', init=Y0, perplexity=30, max_iter=1000)
    kl_host_float32 / kl_host_float64 / kl_host_mixed
                        final KL of chromegcn_amd.tsne.tsne_embed_host from the same start, in its three dtype forms
    kl_bound            kl_sklearn + 3 * (max - min) of those four values: what a correct long run may end at.  A t-SNE
                        trajectory is chaotic, so long runs are compared by the objective they reach, and four correct
                        implementations' own disagreement is the yardstick
    sklearn_version

Needs scikit-learn (the fixture records its version); run from the repository root: python tests/golden/make_tsne_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, D, K, PERPLEXITY, MAX_ITER = 384, 128, 6, 30.0, 1000


def main():
    import sklearn
    from sklearn.manifold import TSNE

    from chromegcn_amd import tsne

    rng = np.random.RandomState(8)
    centres = rng.standard_normal((K, D)) * 1.5
    labels = np.repeat(np.arange(K), N // K)
    X = (centres[labels] + rng.standard_normal((N, D))).astype(np.float32)
    Y0 = (1e-4 * rng.standard_normal((N, 2))).astype(np.float32)
    sk = TSNE(n_components=2, method="exact", init=Y0.copy(), perplexity=PERPLEXITY, max_iter=MAX_ITER, learning_rate="auto")
    sk.fit(X)
    P = tsne.joint_probabilities_host(tsne.sqdist_host(X).astype(np.float32), PERPLEXITY)
    kls = {"kl_sklearn": float(sk.kl_divergence_)}
    for dt in ("float32", "float64", "mixed"):
        kls["kl_host_" + dt] = float(tsne.tsne_embed_host(P, Y0, max_iter=MAX_ITER, dtype=dt)[1]["kl_divergence"])
    spread = max(kls.values()) - min(kls.values())
    kls["kl_bound"] = kls["kl_sklearn"] + 3.0 * spread
    for k, v in kls.items():
        print("%-16s %.6f" % (k, v))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g8_tsne.npz"), X=X, labels=labels.astype(np.int64), Y0=Y0,
                        perplexity=np.float64(PERPLEXITY), max_iter=np.int64(MAX_ITER),
                        sklearn_version=np.array(sklearn.__version__), **{k: np.float64(v) for k, v in kls.items()})


if __name__ == "__main__":
    main()
