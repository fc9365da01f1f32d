"""Names shared by the KSPLSQR step helpers (helper, not a test): the fields of mspi_lsqr_state / mspi_lsqr_dev in
the header's order (tests/test_lsqr_step_layout.py holds them to msplit_internal.h), the s-vectors that go with
the state, and the KSPConvergedReason / convergence-test codes of include/msplit.h."""

# mspi_lsqr_state, field for field
STATE_INTS = ("stop", "reason", "its", "nhist", "i", "max_it", "conv_test", "exact_norm", "hist_cap", "s", "nblk",
              "pad")
STATE_DOUBLES = ("rnorm", "rnorm0", "ttol", "arnorm", "anorm", "alpha", "beta", "phibar", "rhobar", "uscale",
                 "nalpha", "rtol", "abstol", "divtol")
DEV_FIELDS = ("st", "V", "V1", "W", "X", "g", "hist")    # mspi_lsqr_dev
VECTORS = ("V", "V1", "W", "X", "hist")

NANORINF, DTOL, ITS_DIV = -9, -4, -3                     # MSP_DIVERGED_*
RTOL_NORMAL, ATOL_NORMAL, RTOL, ATOL, ITS = 1, 9, 2, 3, 4   # MSP_CONVERGED_*
CONV_DEFAULT, CONV_LSQR, CONV_SKIP = 0, 1, 2             # MSP_LSQR_CONV_*
