"""GPU (-m gpu): every kernel form of the int8 linear GEMM family on operands whose accumulators, and K-split partial sums, fp32 cannot hold (tests/gemm_extremes.py:
> 80 % of the accumulators beyond +-2^24, both signs; one case at the edge of int32), bit for bit against the oracle:
  asq_gemm_i8_i32 (twice; three times on one workspace, tickets back at zero), asq_linear_w8a8 in fp32 at unit scale -- the int -> float conversion itself -- and at
  2^-10, the full epilogue matrix (fp32 / fp16 / bf16 x the eight {s_row, s_col, bias} subsets x both orders, planted +-inf and zero rows), an output whose data
  pointer is not 16-byte aligned, asq_gemm_i8_i8 (half saturated; alpha acc beyond int32 on the edge case), asq_linear_w8a8_q8, the one-launch forward and the
  grouped launch with and without its workspace.
The forms are reached through the library's switches, which are read once per process: one child per environment (gemm_extremes.ENVS), under a timeout; a child that
dies fails its test with the tail of its output, nothing retries.  That each environment reaches the form it is meant to reach, and that an arithmetic fault changes
these outputs but none on uniform random operands, is tests/test_gemm_extremes_cpu.py's subject."""
import pytest

import gemm_extremes as GE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    """operands and exact accumulators of the cases, computed once and shared by the children"""
    return str(tmp_path_factory.mktemp("gemm_extremes"))


@pytest.mark.parametrize("env_name", list(GE.ENVS))
def test_kernel_forms_on_accumulators_beyond_fp32(env_name, cache):
    rc, tail = GE.run_gpu_child(env_name, cache)
    assert rc == 0 and "CHILD OK " + env_name in tail, "environment '%s' (exit status %d):\n%s" % (GE.ENVS[env_name]["env"], rc, tail)
