"""Child process of test_gemm_lattice_exact_under_xcd_map: runs the bf16
lattice GEMM with HS_MOE_XCD=1 (set by the parent in this process's
environment before it starts) and exits non-zero on any mismatch."""

import importlib.util
import pathlib
import sys

here = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(here.parent))

spec = importlib.util.spec_from_file_location(
    "test_moe_gpu", here / "test_moe_gpu.py")
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

if __name__ == "__main__":
    mod.xcd_child_main()
    print("xcd child ok")
