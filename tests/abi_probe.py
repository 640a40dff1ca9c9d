"""What include/proslam_hip.h declares, as the C compiler lays it out: every struct's size and fields, every integer PRS_* constant
and every PRS_API prototype.  A C program generated from the header alone is compiled and run once per process; pure host code.

`python tests/abi_probe.py > tests/golden/abi_v<PRS_ABI_VERSION>.json` records the pin tests/test_abi_layout.py compares against."""
import functools
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "proslam_hip.h")


def header_text():
    return open(HEADER).read()


def _code(header):
    return re.sub(r"/\*.*?\*/", "", header, flags=re.S)


def _declared(header):
    """[(struct, [field, ...])] in declaration order; "int32_t rows, cols;" declares two, "float R[9];" one"""
    out = []
    for body, name in re.findall(r"typedef struct \{([^}]*)\} (prs_\w+);", _code(header)):
        parts = [p for d in body.split(";") for p in d.split(",") if p.strip()]
        out.append((name, [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", p).group(1) for p in parts]))
    return out


def _constant_names(header):
    """object-like #defines and enumerators named PRS_*; PRS_API is the one define that is not an integer"""
    code = _code(header)
    names = [n for n in re.findall(r"^#define (PRS_\w+)[ \t]+\S", code, flags=re.M) if n != "PRS_API"]
    for body in re.findall(r"\benum \{([^}]*)\}", code):
        names += re.findall(r"(?:^|,)\s*(PRS_\w+)", body)
    return names


def prototypes(header=None):
    """{entry point: [return type, [parameter type, ...]]} with the parameter names dropped: "const prs_stereo_params*", "int32_t" """
    def kind(text, named):
        text = re.sub(r"\[[^\]]*\]", "*", text)  # "float X[16]" is passed as a pointer
        stars = text.count("*")
        words = text.replace("*", " ").split()
        if named and len(words) > 1 and words[-1] not in ("int", "float", "double", "char", "void"):
            words = words[:-1]
        return " ".join(words) + "*" * stars

    out = {}
    for ret, name, params in re.findall(r"PRS_API\s+([\w\s\*]+?)\b(prs_\w+)\s*\(([^)]*)\)\s*;", _code(header or header_text())):
        params = [] if params.strip() in ("", "void") else [kind(p, True) for p in params.split(",")]
        out[name] = [kind(ret, False), params]
    return out


def compiler():
    """$CC, cc, or the clang that ships beside hipcc: where the library was built, the last one is always there"""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    beside = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang")
    for cc in (os.environ.get("CC"), "cc", beside):
        if cc and shutil.which(cc.split()[0]):
            return cc.split()
    raise RuntimeError("no C compiler: tried $CC, cc and %s" % beside)


def program(header):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "%s"' % os.path.basename(HEADER), "int main(void) {"]
    for struct, fields in _declared(header):
        lines.append('  printf("S %s %%lu\\n", (unsigned long) sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('  printf("F %s %%lu %%lu\\n", (unsigned long) offsetof(%s, %s), (unsigned long) sizeof(((%s*) 0)->%s));'
                         % (f, struct, f, struct, f))
    for c in _constant_names(header):
        lines.append('  printf("C %s %%lld\\n", (long long) (%s));' % (c, c))
    return "\n".join(lines + ["  return 0;", "}", ""])


@functools.lru_cache(maxsize=None)
def snapshot():
    """{"structs": {name: [size, [[field, offset, size], ...]]}, "constants": {name: value}, "prototypes": {...}}; dicts in header order"""
    header = header_text()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(program(header))
        subprocess.run(compiler() + ["-x", "c", "-std=c99", "-Wall", "-pedantic", "-I", os.path.dirname(HEADER), src, "-o", exe],
                       check=True)
        printed = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    structs, constants = {}, {}
    for tag, name, *numbers in (line.split() for line in printed.splitlines()):
        if tag == "S":
            fields = structs[name] = [int(numbers[0]), []]
        elif tag == "F":
            fields[1].append([name, int(numbers[0]), int(numbers[1])])
        else:
            constants[name] = int(numbers[0])
    return {"structs": structs, "constants": constants, "prototypes": prototypes(header)}


def dumps(snap):
    """one struct, one prototype per line, so that a diff of the pin reads as a layout change"""
    def section(d):
        return "{\n" + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in d.items()) + "\n }"
    return "{\n" + ",\n".join(' %s: %s' % (json.dumps(k), section(v)) for k, v in snap.items()) + "\n}\n"


if __name__ == "__main__":
    sys.stdout.write(dumps(snapshot()))
