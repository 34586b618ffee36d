#!/usr/bin/env python3
"""Resource and fast-block census of EVERY packed-fp16 specialised score kernel of a kernel cache, without a GPU: each
kernel is recompiled to a listing (hipcc -S) from the given pc_jit_source.h with the options its cache file records; the
block-resolved (fast) block is the basic block with the most v_pk_maximum3_f16.  One line per kernel: the row its row-skipping
fast path tests (r0 = R: the plain kernel), its layout (top = 1: the shorter adapter top-aligned, with the K_up terms its
fast path fetches per column; else K_up = K), registers, scratch, LDS, occupancy (the compiler's, which counts LDS in), and the
block's VALU instructions, scratch instructions, register moves and s_nops.
   python tools/panel_isa.py [porechop_amd/csrc/pc_jit_source.h [porechop_amd/kernel_cache]] > panel.txt"""
import os, re, shutil, subprocess, sys, collections, tempfile
from concurrent.futures import ThreadPoolExecutor
HERE = os.path.dirname(os.path.abspath(__file__))
src_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "porechop_amd", "csrc", "pc_jit_source.h")
cache = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "..", "porechop_amd", "kernel_cache")
src = open(src_path).read()
src = src[src.index('R"PCJIT(') + 8: src.index(')PCJIT"')]
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
tmpd = tempfile.mkdtemp()
p = os.path.join(tmpd, 'k.hip'); open(p, 'w').write('#include <hip/hip_runtime.h>\n' + src)
jobs = {}
for f in sorted(os.listdir(cache)):
    if not f.endswith('.pcjk'): continue
    b = open(os.path.join(cache, f), 'rb').read()
    hdr = b[:b.find(b'\x7fELF')].decode('latin1')
    defs = re.findall(r'-DPC_[A-Z_0-9]+=[^\s\x00]+', hdr)
    if '-DPC_F16=1' not in defs: continue
    jobs[' '.join(defs)] = defs
def run(defs):
    res = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', '-', p] + defs,
                         capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (' '.join(defs), res.stderr[-2000:]))
    out = res.stdout
    blocks, cur = [], ['entry', []]
    for l in out.split('\n'):
        if re.match(r'^\.LBB\d+_\d+:', l): blocks.append(cur); cur = [l.split(':')[0], []]
        else:
            s = l.split(';')[0].strip()
            if s and not s.startswith('.'): cur[1].append(s)
    blocks.append(cur)
    best = max(blocks, key=lambda b: sum(i.startswith('v_pk_maximum3_f16') for i in b[1]))
    c = collections.Counter(i.split()[0] for i in best[1])
    g = lambda k: int(re.search(r'; %s: (\d+)' % k, out).group(1))
    d = dict(x[2:].split('=', 1) for x in defs)
    return (int(d['PC_R']), int(d['PC_K']), int(d['PC_WAVES']), int(d['PC_DUAL']), int(d.get('PC_R0', d['PC_R'])), int(d.get('PC_TOP', 0)), int(d.get('PC_KUP', d['PC_K'])), g('NumVgprs'), g('NumAgprs'), g('ScratchSize'),
            g('LDSByteSize'), g('Occupancy'),
            c['v_pk_maximum3_f16'], sum(v for k, v in c.items() if k.startswith('v_')), sum(v for k, v in c.items() if k.startswith('scratch_')),
            c['v_mov_b32_e32'] + c.get('v_accvgpr_read_b32', 0) + c.get('v_accvgpr_write_b32', 0), c['s_nop'])
try:
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        res = list(ex.map(run, jobs.values()))
finally:
    shutil.rmtree(tmpd, ignore_errors=True)
print('R K waves dual r0 top K_up vgpr agpr scratchB ldsB occupancy | fast block: max3 VALU scratch_instrs moves s_nop')
for r in sorted(res): print(*r)
