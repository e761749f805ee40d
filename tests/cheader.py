"""What a public header declares, for the tests that hold the ctypes binding against it."""
import re


def prototypes(header):
    """name -> (return type, number of parameters) of every APE_LZ4_ function the header file
    declares, comments and macros dropped."""
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"#define[^\n]*(\\\n[^\n]*)*", "", src)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w \t\n\*]*?)\b(APE_LZ4_\w+)\s*\(([^()]*)\)\s*;", src):
        params = m.group(3).strip()
        protos[m.group(2)] = (" ".join(m.group(1).split()),
                              0 if params in ("", "void") else params.count(",") + 1)
    return protos
