"""Resume of a run whose pinball fits run on Levenberg-Marquardt, on the HIP
backend: the GPU twin of test_api_features.test_resume_lm_pinball_restores_
gram_values at 2^12 paths.  The resumed run rebuilds ``gvalues[5]`` (the Gram-
subsample targets of its first pinball fit) with the eval epilogue's n_local-
override calls from the restored networks.

Measured on an MI355X: max|resumed - full| of gvalues[5] 7.2e-7 at max|V| 4.37
(weight round trip 5.8e-7 in fp64, tolerance 1.7e-5)."""
import pytest

from test_api_features import check_lm_resume
from test_gpu_kernels import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_resume_lm_pinball_restores_gram_values_gpu(dev, tmp_path):  # noqa: F811
    check_lm_resume(tmp_path, dev, 12)
