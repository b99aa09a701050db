"""CPU guard read off the ISA (hipcc cross-compiles for gfx950, no GPU): the wave-private azimuth tile kernel of az_wave.hip
keeps the shape it was built for - every instance has no LDS (group segment 0), no s_barrier, no scratch, at most 256 VGPRs
(two waves per SIMD), and issues all of its image loads before it waits for the first one."""
import os
import re
import subprocess
import sys
import tempfile

from conftest import ROOT

SRC = os.path.join(ROOT, "nis-sar-amtigmti-video_amd", "csrc", "az_wave.hip")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize", "-S", "--cuda-device-only"]


def _asm():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-I", os.path.dirname(SRC), SRC, "-o", out], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def test_wave_tiles_have_no_lds_barrier_or_scratch():
    text = _asm()
    descs = dict(re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S))
    names = [k for k in descs if "az_wave_kernel" in k]
    assert len(names) == 16, names          # {fwd, inv} x epilogue x {nt, plain} x {1, 4} waves per workgroup
    for name in names:
        d = descs[name]
        field = lambda f: int(re.search(r"\.amdhsa_%s (\d+)" % f, d).group(1))
        assert field("group_segment_fixed_size") == 0, name
        assert field("private_segment_fixed_size") == 0, name
        assert field("next_free_vgpr") <= 256, (name, field("next_free_vgpr"))
        body = re.search(r"^%s:.*?^\s*s_endpgm" % re.escape(name), text, re.S | re.M).group(0)
        assert "s_barrier" not in body, name
        assert not re.search(r"^\s*ds_(read|write|load|store)", body, re.M), name     # (the max reduction's ds_bpermute is no LDS image)
        assert body.count("v_permlane32_swap") == 128, name     # two exchanges of 32 register pairs, re and im


def test_wave_tiles_issue_their_loads_together():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_load_waits
    rows = [r for r in isa_load_waits.census(SRC) if "az_wave_kernel" in r[0]]
    assert len(rows) == 16
    for name, loads, stores, waits, waits0, serial in rows:
        assert loads in (64, 66) and stores in (64, 65), (name, loads, stores)     # + two c1 rows per lane (PHI1), + the max atomic (SCALE)
        assert serial <= 1, (name, serial)
