"""The preconditioner on Neumann and Robin faces, piece by piece against something that is not itself:
the checks of tests/boundary_checks.py with every term, on the GPU.  tests/test_gpu_boundary.py holds the outer solution to
the assembled matrix; an outer FCG / GMRES meets that with a preconditioner that is wrong on every boundary dof, in more
steps.  Here

  the inner operator and its exact diagonal   Reference.K_free() in the numbering of sub_point_dofs, 1e-12 (the bound of
                                              test_node_operator_is_the_matrix and diffusivity_checks.check_operator)
  the level-0 low-order matrix                the restatement of low_order::assemble_fem on the problem's point -> dof array
                                              plus cbar on the diagonal, as bits (diffusivity_checks.check_hierarchy_matrix)
  the V-cycle, the inner and the outer solve  the oracle, which reads p_mask from the mesh it is given: 1e-11, 1e-9, 1e-8 and
                                              its iteration count (amg_checks, unchanged; no cap on the count)

No bound is new.  The CPU twins (tests/test_cpu_boundary.py) run the same functions on the stand-in of the kernel library,
without lambda and alpha, which that library lacks; measured figures and times are in tests/README.md."""
import pytest

import boundary_checks as B
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(gpu):
    """the library's own stream, as tests/test_gpu_amg.py and test_gpu_amg_device_setup.py run these checks"""
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    yield True
    H.init(0)


@pytest.mark.parametrize("case", list(B.OPERATOR_CASES))
def test_inner_operator_and_its_diagonal_are_the_matrix(setup, case):
    B.check_inner_operator(case)


@pytest.mark.parametrize("case", list(B.HIERARCHY_CASES))
def test_level0_matrix_is_its_restatement_as_bits(setup, case):
    B.check_level0_matrix(case)


@pytest.mark.parametrize("case", list(B.ORACLE_CASES))
def test_vcycle_and_solves_are_the_oracles(setup, case):
    B.check_against_oracle(case)
