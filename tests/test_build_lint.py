"""The built HIP library must not hold the 64-bit shift form that MI355X executes wrongly (tools/isa_lint.py: a shift amount in the
last register of the wave's VGPR allocation), and the lint itself must find that form where it is known to be.  CPU only:
hipcc cross-compiles and llvm-objdump disassembles without a GPU."""
import os
import subprocess

import pytest

from support import ROOT


def test_the_built_library_holds_no_shift_by_the_last_allocated_register():
    import __graft_entry__ as g
    from tools import isa_lint
    g.build()
    kernels, checked, found = isa_lint.lint(g.HIP_LIB)
    assert kernels >= 30 and checked > 100, "the lint did not see the library's kernels"
    assert found == [], f"hazardous 64-bit shifts in the built library: {found}"


def test_the_lint_finds_the_form_in_the_hardware_probe(tmp_path):
    """tools/probes/shift64_top.hip builds that form on purpose (inline assembler): seven of its kernels shift by the last register"""
    import __graft_entry__ as g
    from tools import isa_lint
    co = str(tmp_path / "probe.co")
    subprocess.check_call([g._hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-O2", "-c",
                           os.path.join(ROOT, "tools", "probes", "shift64_top.hip"), "-o", co], stderr=subprocess.DEVNULL)
    _kernels, checked, found = isa_lint.lint(co)
    names = sorted(k for k, _vg, _al, _ins in found)
    assert checked >= 12
    assert len(found) == 7, names                    # shl/lshr/ashr of v15, and shl of v23, v31, v63, v127
    assert not any("v14" in k or "sub" in k or "mad" in k or "cvt" in k for k in names), names


def test_the_tile_kernel_keeps_the_properties_its_build_flags_buy():
    """The frame time rests on eight code-generation switches (__graft_entry__.HIPCC_TUNING) that keep the tile kernel's main
    instantiations inside 96 vector registers with next to no scratch traffic (at 128 registers the next frame's
    set-up pass no longer fits beside it, +12 %; a reload per pulled block cost 2-6 %).  A compiler bump that silently loses them fails
    HERE instead of in a benchmark: for k_tile<*, COMPLETE = false, FAST = true, *> -- the launches that draw the frames --
    VGPRs <= 96, scratch <= 48 bytes per lane (a dozen values parked at kernel entry and reloaded once per work item), and no scratch access inside the chunk loop or below it (loop depth >= 2: the block
    pull loop, pass A / B, the line loop, painting)."""
    from tools import isa_stats                              # recompiles vf_hip.hip with the build's flags + --save-temps (about 30 s)
    _text, records, depths = isa_stats.collect()
    mains = {k: v for k, v in records.items() if k.startswith("k_tile<") and k.split(", ")[1] == "false" and k.split(", ")[2] == "true"}
    assert len(mains) == 4, sorted(records)
    for name, nt in mains.items():
        assert int(nt["NumVgprs"]) <= 96, (name, nt)
        assert int(nt["ScratchSize"]) <= 48, (name, nt)
        assert int(nt["Occupancy"]) >= 5, (name, nt)
        assert int(nt["LDSByteSize"]) <= 81920, (name, nt)       # half a CU's LDS: beyond it the register budget is silently dropped
    assert set(depths) == {"k_tile<false, false, true, true>", "k_tile<false, false, true, false>"}
    for name, hist in depths.items():
        deep = {k: n for k, n in hist.items() if k[0] >= 2}
        assert not deep, f"{name}: scratch accesses inside the chunk loop or below: {deep}"
    # the set-up pass must fit beside the tile kernel: 512 - 4 waves x 96 registers leave 128 per SIMD
    assert int(records["k_block_setup"]["NumVgprs"]) <= 64, records["k_block_setup"]


def test_build_survives_a_compiler_that_refuses_a_tuning_switch(tmp_path, monkeypatch):
    """the eight -mllvm switches are LLVM internals.  A ROCm that renames one must cost the tuning, not the round:
    the compile is repeated without them, build_info.json records `tuning_flags_applied: false`, and the library works (here: it
    loads and exports the C-ABI; no GPU needed).  Everything is redirected to a scratch directory -- the in-tree library stays."""
    import ctypes
    import json

    import __graft_entry__ as g
    lib, info = str(tmp_path / "libvf_hip.so"), str(tmp_path / "build_info.json")
    monkeypatch.setattr(g, "HIP_LIB", lib)
    monkeypatch.setattr(g, "BUILD_INFO", info)
    applied, note = g._compile_hip(tuning=[*g.HIPCC_TUNING, "-mllvm", "-vf-no-such-switch-in-this-llvm"])
    assert applied is False and note and "vf-no-such-switch" in note
    g._lint(lib)
    g._write_build_info(applied, note)
    rec = json.load(open(info))
    assert rec["tuning_flags_applied"] is False and "-mllvm" not in rec["flags"] and rec["note"]
    h = ctypes.CDLL(lib)
    assert h.vf_terrain_render and h.vf_ctx_create
