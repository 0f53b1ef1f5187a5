"""Instruction mix per kernel from the gfx950 assembly (metalbt709decoder_amd/build/*.s).
usage: python tools/isa_mix.py [file.s]
       python tools/isa_mix.py --compare parent.s result.s [name-regex]

--compare: two assemblies of the same kernels -- build.emit_asm() on the parent commit's tree and on the result's -- paired by
ROLE: the demangled kernel name with the chroma layout taken out of it, whether it is spelled in the name (decode_nv12_quads<..>,
encode_bgra_i420, encode_alpha_y_blocks_i420) or is the leading unsigned template argument (decode_quads<0u, ..>, encode_bgra<1u>),
so a kernel keeps its role across a rename of that kind (a parent kernel that names no layout pairs with the result's NV12 one).
Per kernel (those whose role matches name-regex): `identical` when the instruction streams are equal with .LBB<n>_ labels
normalised and the metadata is; else the number of differing lines (a line diff), every opcode whose count differs, the number of
s_waitcnt with a vmcnt field, VGPRs, SGPRs and scratch bytes, parent then result."""
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys


def mix(path):
    s = open(path).read()
    parts = re.split(r'\n(_Z\w+):[^\n]*\n', s)
    for i in range(1, len(parts), 2):
        name = parts[i]
        body = parts[i + 1].split('s_endpgm')[0]
        ins = [l.split()[0] for l in body.split('\n') if l.startswith('\t') and l.strip() and not l.strip().startswith(('.', ';'))]
        c = collections.Counter()
        for k in ins:
            if k.startswith('v_'):
                c['valu'] += 1
            elif k.startswith(('ds_', 'global_', 'buffer_')):
                c[k] += 1
            elif k.startswith('s_waitcnt'):
                c['waitcnt'] += 1
            elif k.startswith('s_'):
                c['salu'] += 1
        print(name[:70], len(ins), dict(c))


def demangle(symbols):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")
    out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(symbols, out))


def role(demangled):
    """'void bt709::decode_nv12_quads<false, true, false>(bt709::DecodeParams)' and '... decode_quads<0u, false, true, false>(...)'
    -> 'decode_quads[nv12]<false, true, false>'."""
    m = re.match(r"(?:void )?(?:bt709::)?(\w+)(?:<(.*)>)?\(", demangled)
    func, args = m.group(1), [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
    layout = None
    for tag in ("nv12", "i420"):
        if re.search(r"_%s(_|$)" % tag, func):
            layout, func = tag, re.sub(r"_%s(?=_|$)" % tag, "", func)
    if layout is None and args and args[0] in ("0u", "1u"):
        layout = ("nv12", "i420")[int(args.pop(0)[0])]
    return "%s%s%s" % (func, "[%s]" % layout if layout else "", "<%s>" % ", ".join(args) if args else "")


def kernels(path):
    """role -> (instruction lines, metadata) of every kernel of an assembly file."""
    s = open(path).read()
    bodies = dict(re.findall(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", s, flags=re.S | re.M))
    meta = {}
    for entry in re.split(r"^  - \.agpr_count:", s, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)
        meta[name] = {k: int(re.search(r"^    \.%s:\s+(\d+)" % k, entry, re.M).group(1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")}
    names = demangle(sorted(n for n in bodies if n in meta))
    out = {}
    for sym, dem in names.items():
        ins = []
        for line in bodies[sym].split("\n"):
            line = line.split(";")[0].rstrip()
            if line.startswith("\t") and not line.strip().startswith("."):
                ins.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())).replace(sym, "<self>"))
        r = role(dem)
        assert r not in out, r
        out[r] = (ins, meta[sym])
    return out


def compare(parent_path, result_path, pattern):
    parent, result = kernels(parent_path), kernels(result_path)
    for r in [r for r in parent if "[" not in r and r not in result]:  # a kernel that named no layout (encode_alpha_y) was the NV12 one
        tagged = re.sub(r"^(\w+)", r"\1[nv12]", r)
        if tagged in result:
            parent[tagged] = parent.pop(r)
    chosen = sorted(r for r in set(parent) | set(result) if re.search(pattern, r))
    identical = 0
    for r in chosen:
        if r not in parent or r not in result:
            print("%-58s ONLY IN THE %s" % (r, "PARENT" if r in parent else "RESULT"))
            continue
        (a, ma), (b, mb) = parent[r], result[r]
        if a == b and ma == mb:
            identical += 1
            print("%-58s identical (%d instructions, vgpr %d sgpr %d scratch %d)" % (r, len(a), ma["vgpr_count"], ma["sgpr_count"], ma["private_segment_fixed_size"]))
            continue
        changed = sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
        ca, cb = collections.Counter(i.split()[0] for i in a), collections.Counter(i.split()[0] for i in b)
        ops = ", ".join("%s %d -> %d" % (k, ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]) or "none"
        vm = [sum(1 for i in x if i.startswith("s_waitcnt") and "vmcnt" in i) for x in (a, b)]
        print("%-58s %d lines differ (%d -> %d instructions); opcode counts that differ: %s; vmcnt waits %d -> %d; vgpr %d -> %d; sgpr %d -> %d; scratch %d -> %d" % (
            r, changed, len(a), len(b), ops, vm[0], vm[1], ma["vgpr_count"], mb["vgpr_count"], ma["sgpr_count"], mb["sgpr_count"],
            ma["private_segment_fixed_size"], mb["private_segment_fixed_size"]))
    print("# %d kernels compared, %d identical" % (len(chosen), identical))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "")
    else:
        mix(sys.argv[1] if len(sys.argv) > 1 else "metalbt709decoder_amd/build/bt709_kernels.s")
