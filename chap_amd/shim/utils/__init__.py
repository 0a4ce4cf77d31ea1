"""`utils` shim, beside the `networks` one: with `chap_amd/shim` on PYTHONPATH `from utils.test_3d_patch import test_all_case`
(code/test_LA.py:5) resolves to chap_amd.test_3d_patch.  The reference's own `utils/` package is absent upstream;
only the module test_LA.py needs is supplied."""
