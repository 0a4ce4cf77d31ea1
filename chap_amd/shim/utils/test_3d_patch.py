from chap_amd.test_3d_patch import (calculate_metric_percase, getLargestCC, test_all_case, test_single_case_average_output,  # noqa: F401
                                    test_single_case_first_output, var_all_case, window_origins)

__test__ = False      # the reference's function names, not pytest's
