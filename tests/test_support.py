"""tests/support.py's build_sim decides from the compiler's own dependency record, the command line and the files' times whether
a simulator library is rebuilt: a two-file simulator in tmp_path, through every reason for a rebuild."""
import ctypes as C
import os
import shutil

from support import build_sim


def test_build_sim_rebuilds_when_a_header_the_flags_or_the_record_change(tmp_path):
    (tmp_path / "toy_value.h").write_text("#define TOY_VALUE 41\n")
    (tmp_path / "toy.cpp").write_text('#include "toy_value.h"\nextern "C" int toy() { return TOY_VALUE + TOY_ADD; }\n')
    so, rec = str(tmp_path / "libtoy.so"), str(tmp_path / "libtoy.so.d")
    loads = []

    def build(flags=("-DTOY_ADD=0",)):
        """-> (what a FRESH load of the library returns -- a copy under a new name: dlopen hands back a loaded library by name --,
        the library file's identity)"""
        assert build_sim("toy", flags=flags, src_dir=tmp_path, out_dir=tmp_path)._name == so
        loads.append(str(tmp_path / ("load%d.so" % len(loads))))
        shutil.copy(so, loads[-1])
        st = os.stat(so)
        return C.CDLL(loads[-1]).toy(), (st.st_ino, st.st_mtime_ns)

    v, first = build()
    assert v == 41 and os.path.exists(rec)
    assert sorted(os.listdir(tmp_path)) == ["libtoy.so", "libtoy.so.d", "load0.so", "toy.cpp", "toy_value.h"]   # no temporary left
    assert build() == (41, first)                              # unchanged: the same file
    # the header changes and is newer than the library
    (tmp_path / "toy_value.h").write_text("#define TOY_VALUE 42\n")
    t = os.stat(so).st_mtime_ns + 2 * 10 ** 9
    os.utime(tmp_path / "toy_value.h", ns=(t, t))
    v, second = build()
    assert v == 42 and second != first
    os.utime(so, ns=(t, t))                                    # (the library as new as the header: fresh again)
    second = (second[0], t)
    assert build() == (42, second)
    # other flags, nothing else changed
    v, third = build(("-DTOY_ADD=100",))
    assert v == 142 and third != second
    os.utime(so, ns=(t, t))
    assert build(("-DTOY_ADD=100",)) == (142, (third[0], t))
    # the record is gone; then unreadable
    os.remove(rec)
    v, fourth = build(("-DTOY_ADD=100",))
    assert v == 142 and fourth[0] != third[0] and os.path.exists(rec)
    os.utime(so, ns=(t, t))
    open(rec, "w").write("{")
    v, fifth = build(("-DTOY_ADD=100",))
    assert v == 142 and fifth[0] != fourth[0]
