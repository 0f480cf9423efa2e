"""Recipe for oracle/_ref/ (untracked): compiled copies of upstream FasterViT files that tests run unmodified.

The upstream checkout is read only here, at build time; tests read what this recipe left under oracle/_ref/ and skip
when it is absent.  Its location is FVIT_REFERENCE_DIR, by default the build container's checkout (the same one
tests/golden/make_golden.py reads).

  fastervit/validate.py -> oracle/_ref/validate.pyc   (tests/test_validate_dropin.py: the reference's own eval script
                                                      driving this package through scripts/run_reference_validate.py)
"""
import os
import py_compile

REF_DIR = os.environ.get("FVIT_REFERENCE_DIR", "/root/reference")
OUT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref")
FILES = {"validate.pyc": os.path.join("fastervit", "validate.py")}


def build() -> list:
    """Compile every file of FILES that the upstream checkout has; returns the paths written (empty without a checkout)."""
    made = []
    for out, src in FILES.items():
        src = os.path.join(REF_DIR, src)
        if not os.access(src, os.R_OK):
            continue
        os.makedirs(OUT_DIR, exist_ok=True)
        made.append(py_compile.compile(src, cfile=os.path.join(OUT_DIR, out), doraise=True))
    return made


if __name__ == "__main__":
    print("\n".join(build()) or "no upstream checkout at " + REF_DIR)
