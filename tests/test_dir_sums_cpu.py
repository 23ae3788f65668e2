"""The SH direction sums without a GPU: one new entry point, no ABI bump, the library exports it and the Python binding
reaches it; the two counters behind the existing twelve."""
import inspect
import os
import re

from conftest import ROOT, pkg


def test_entry_point_is_declared_exported_and_bound():
    lib_mod = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define\s+GSPLAT_ABI_VERSION\s+9\b", header) and lib_mod.ABI_VERSION == 9, "new entry point only: no ABI bump"
    assert re.search(r"\bint\s+gsplat_context_set_dir_sums\s*\(\s*gsplat_context\s*\*\s*ctx\s*,\s*int\s+enabled\s*\)", header)
    assert lib_mod.SIGNATURES["gsplat_context_set_dir_sums"] == lib_mod.SIGNATURES["gsplat_context_set_compact_lists"]
    lib_mod.build()
    lib = lib_mod.load()
    assert hasattr(lib, "gsplat_context_set_dir_sums"), "declared but not exported"
    assert lib.gsplat_abi_version() == 9
    assert lib.gsplat_context_set_dir_sums(None, 1) != 0  # (a null context is refused, not dereferenced)
    raster = pkg("raster")
    assert list(inspect.signature(raster.RasterContext.set_dir_sums).parameters) == ["self", "enabled"]
    src = inspect.getsource(raster.RasterContext.counters)
    assert "dir_sums_backwards=int(v[12])" in src and "dir_sums_fallbacks=int(v[13])" in src


def test_switches_are_documented_where_the_others_are():
    ctx_h = open(os.path.join(ROOT, "3dgs_amd", "csrc", "gs_context.h")).read()
    ctx_src = open(os.path.join(ROOT, "3dgs_amd", "csrc", "gs_context.hip")).read()
    assert "GSPLAT_NO_DIR_SUMS" in ctx_h and 'env_is("GSPLAT_NO_DIR_SUMS", \'1\')' in ctx_src
    assert re.search(r"f\(c\.dir_sums, W\)", ctx_h), "the buffer must be in the context's buffer table"
