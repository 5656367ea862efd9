"""Compare kernels of two device assemblies (`hipcc ... --cuda-device-only -S`) instruction for instruction -- comments, label numbers and
the kernel's own symbol ignored -- and by their VGPR, AGPR, SGPR, LDS and scratch metadata.  One line per kernel; exit status 1 when
a pair differs.  Without names: every kernel of A against the kernel of the same name in B.
Usage: python tools/kernel_asm_diff.py A.s B.s [name | name_in_A=name_in_B ...]     (names as c++filt prints them, without namespace
and arguments: stats_kernel, 'conv3x3_mfma_kernel<2>')"""
import re
import shutil
import subprocess
import sys

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    out = {}
    for entry in text.split("amdhsa.kernels:")[1].split("amdhsa.target")[0].split("\n  - .agpr_count")[1:]:
        entry = ".agpr_count" + entry
        sym = re.search(r"\.name:\s+(\S+)", entry).group(1)
        body = re.split(r"^" + re.escape(sym) + r":.*$", text, 1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()).replace(sym, "SELF") for l in body.split("\n")]
        lines = [l for l in lines if l.strip()]
        meta = {k: int(re.search(r"\." + k + r":\s+(\d+)", entry).group(1)) for k in KEYS}
        name = subprocess.run([shutil.which("c++filt") or shutil.which("llvm-cxxfilt"), sym], capture_output=True, text=True).stdout.strip()
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out[name] = (lines, meta)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
pairs = [p.split("=") if "=" in p else (p, p) for p in sys.argv[3:]] or [(k, k) for k in a]
differ = False
for ka, kb in pairs:
    (la, ma), (lb, mb) = a[ka], b[kb]
    print(f"{ka} / {kb}: instructions {'same' if la == lb else 'DIFFER'} ({len(la)} / {len(lb)}), metadata {'same' if ma == mb else 'DIFFER'} "
          + " ".join(f"{k.split('_')[0]} {ma[k]}" + ("" if ma[k] == mb[k] else f" -> {mb[k]}") for k in KEYS))
    differ |= la != lb or ma != mb
sys.exit(1 if differ else 0)
