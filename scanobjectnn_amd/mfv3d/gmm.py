"""The fixed grid mixture of 3DmFV-Net -- `3DmFV-Net/utils/utils.py:69-92` (get_3d_grid_gmm) without sklearn: the model
only ever reads weights_, means_ and sqrt(covariances_) of the GaussianMixture object (`train.py:278-283`)."""
import numpy as np


def get_3d_grid_gmm(subdivisions=(5, 5, 5), variance=0.04):
    """-> (w (K,), mu (K, 3), sigma (K, 3)) float64, K = prod(subdivisions), first axis slowest.
    `np.mgrid[step - 1:1 - step:complex(0, n)]` (utils.py:80-82) is linspace(step - 1, 1 - step, n) with step = 1 / n;
    sigma is the STANDARD DEVIATION sqrt(variance), what the reference feeds as sigma_pl."""
    if isinstance(subdivisions, int):
        subdivisions = (subdivisions,) * 3
    n = [int(s) for s in subdivisions]
    if len(n) != 3 or min(n) < 1:
        raise ValueError("subdivisions must be three positive integers, got %r" % (subdivisions,))
    axes = [np.linspace(1.0 / s - 1.0, 1.0 - 1.0 / s, s) for s in n]
    mu = np.stack(np.meshgrid(*axes, indexing="ij"), axis=0).reshape(3, -1).T.copy()
    k = mu.shape[0]
    w = np.full(k, 1.0 / k)
    sigma = np.sqrt(float(variance) * np.ones_like(mu))
    return w, mu, sigma
