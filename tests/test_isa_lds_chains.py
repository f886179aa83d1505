"""A guard on what the compiler does with the LDS reads of parallel_shuffle (DESIGN section 3.1
item 6): tests/cpp/shuffle_probe.hip, which instantiates the routine with and without its block
mask, is compiled to assembly with the product's flags and read by tools/isa_serial_loads.py
--lds: no chain of four or more LDS reads that are each waited for (s_waitcnt lgkmcnt(0)) before
the next one is issued, in either instance.

Four, because the routine's longest stretch of dependent single reads is three: the gather is
three dependent groups (first depositor and partner; the end of the depositor's chain; the
source's value) and a pointer-jumping pass is two.  With a guard on every element the compiler
put each read of the gather's last group into an exec-mask block with a wait of its own: a chain
of eight, which this test fails on.  CPU only (hipcc cross-compiles).  The product's instance
<4, 2, 2> takes minutes to compile and is audited by hand with the same tool."""
import os
import subprocess
import sys

import pytest

import shuffle_probe_lib as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CHAIN = 4


@pytest.mark.skipif(not os.path.exists(P.HIPCC), reason="no hipcc")
def test_no_chain_of_self_waited_lds_reads(tmp_path):
    asm = P.compile_probe(str(tmp_path / "shuffle_probe.s"), ["-gline-tables-only", "-S", "--cuda-device-only"])
    tool = os.path.join(ROOT, "tools", "isa_serial_loads.py")
    every = subprocess.run([sys.executable, tool, asm, "1", "--lds"], check=True, capture_output=True,
                           text=True).stdout.splitlines()
    # the tool saw both instances and their LDS reads at all
    for inst in ("shuffle_kernelILb0E", "shuffle_kernelILb1E"):
        assert any(inst in l and "ds_read" in l for l in every), inst
    out = subprocess.run([sys.executable, tool, asm, str(MIN_CHAIN), "--lds"], check=True, capture_output=True,
                         text=True).stdout
    chains = [l for l in out.splitlines() if "ds_read" in l]
    assert not chains, "\n".join(chains)


def test_default_report_is_unchanged_by_the_lds_mode(tmp_path):
    """the tool on a hand-written listing: global loads by default, LDS reads only on request"""
    asm = tmp_path / "toy.s"
    asm.write_text("\n".join([
        "toy:",
        "\tglobal_load_dword v1, v0, s[0:1]", "\ts_waitcnt vmcnt(0)",
        "\tglobal_load_dword v2, v1, s[0:1]", "\ts_waitcnt vmcnt(0)",
        "\tds_read_b32 v3, v2", "\ts_waitcnt lgkmcnt(0)",
        "\tds_read_b32 v4, v3", "\ts_waitcnt lgkmcnt(0)",
        "\tds_read_b32 v5, v4", "\tds_read_b32 v6, v4", "\ts_waitcnt lgkmcnt(0)",
        "\tds_read_b32 v7, v5", "\ts_waitcnt lgkmcnt(0)",
        "\ts_endpgm",
        "\t.amdhsa_kernel toy",
    ]) + "\n")
    tool = os.path.join(ROOT, "tools", "isa_serial_loads.py")
    run = lambda *a: subprocess.run([sys.executable, tool, str(asm)] + list(a), check=True, capture_output=True,
                                    text=True).stdout.splitlines()
    plain = run()
    assert len(plain) == 1 and "chain 2" in plain[0] and "global_load_dword" in plain[0] and "ds_read" not in plain[0]
    lds = run("1", "--lds")
    # two self-waited reads; the pair in flight together ends the run; its last read and the next one
    assert [l.split("chain ")[1].split()[0] for l in lds] == ["2", "2"]
    assert all("ds_read_b32" in l and "global_load" not in l for l in lds)
    assert run("3", "--lds") == []
