"""CPU: the lab hooks of the pruned batch on the 5-bit shadow are declared in the debug header, bound in
_lib._DEBUG_SIGNATURES and exported by the lab build alone."""
import subprocess

from seesaw_amd import _lib

HOOKS = {"ssw_tune_prune5_batch", "ssw_debug_prune5_bounds_mq", "ssw_debug_prune5_survivors_mq"}


def exported(path):
    return {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", path], check=True,
                                                        capture_output=True, text=True).stdout.splitlines() if line}


def test_hooks_are_declared_bound_and_exported_in_the_lab_build_only():
    assert (HOOKS <= set(_lib.declared_symbols(_lib.DEBUG_HEADER_PATH)) and HOOKS <= set(_lib._DEBUG_SIGNATURES)
            and HOOKS <= exported(_lib.DEBUG_LIB_PATH) and not HOOKS & set(_lib.declared_symbols())
            and not HOOKS & set(_lib._SIGNATURES) and not HOOKS & exported(_lib.LIB_PATH))
