"""cabi.parse on short header texts: what the two headers contain parses, and
anything the reader does not fully understand raises (it never guesses)."""
import ctypes

import pytest

import cabi

GOOD = """
/* a block
   comment */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define T_VERSION 7 /* trailing
                       comment */
#define T_MAX 3
#define T_HEX 0x10
#define T_LIVE(slot) (1 << (slot))
enum t_kind { T_A = 0, T_B, T_C = 5, T_D };
struct t_later;
typedef struct t_inner {
  uint16_t* data;
  int64_t rows, ld;
} t_inner;
typedef struct t_outer {
  const float* y;
  int n;
  t_inner plane;            /* by value */
  float thr[T_MAX];
  void* dst[T_MAX];         /* array of pointers */
  int32_t elem[2];
  float a, b;
  const struct t_later* next;
  size_t bytes;
  double g;
  uint32_t u;
  uint64_t* seed;
} t_outer;
typedef struct t_later {
  int live;
} t_later;
int t_version(void);
const char* t_last_error(void);
size_t t_bytes(const t_shape* shape, int gemm);
int64_t t_cols(int64_t n);
int t_run(const t_outer* args, const char* tag, float* out /* (n) */, double scale,
          uint64_t seed, const uint8_t* mask, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def parse_text(tmp_path, text, known=None):
    path = tmp_path / "t.h"
    path.write_text(text)
    return cabi.parse(str(path), known)


def test_tolerated_constructs_parse(tmp_path):
    class t_shape(ctypes.Structure):
        _fields_ = [("B", ctypes.c_int64)]

    h = parse_text(tmp_path, GOOD, {"t_shape": t_shape})
    # object-like integer defines and enumerators; the guard and T_LIVE(slot) are not constants
    assert h.constants == {"T_VERSION": 7, "T_MAX": 3, "T_HEX": 16,
                           "T_A": 0, "T_B": 1, "T_C": 5, "T_D": 6}
    assert list(h.structs) == ["t_inner", "t_outer", "t_later"]
    inner, outer = h.structs["t_inner"], h.structs["t_outer"]
    vp = ctypes.c_void_p
    assert inner._fields_ == [("data", vp), ("rows", ctypes.c_int64), ("ld", ctypes.c_int64)]
    assert outer._fields_ == [
        ("y", vp), ("n", ctypes.c_int), ("plane", inner), ("thr", ctypes.c_float * 3),
        ("dst", vp * 3), ("elem", ctypes.c_int32 * 2), ("a", ctypes.c_float),
        ("b", ctypes.c_float), ("next", vp), ("bytes", ctypes.c_size_t), ("g", ctypes.c_double),
        ("u", ctypes.c_uint32), ("seed", vp)]
    assert outer.plane.offset == 16 and outer.thr.offset == 40 and ctypes.sizeof(outer) == 136
    assert h.prototypes == {
        "t_version": (ctypes.c_int, []),
        "t_last_error": (ctypes.c_char_p, []),
        "t_bytes": (ctypes.c_size_t, [ctypes.POINTER(t_shape), ctypes.c_int]),
        "t_cols": (ctypes.c_int64, [ctypes.c_int64]),
        "t_run": (ctypes.c_int, [ctypes.POINTER(outer), ctypes.c_char_p, vp, ctypes.c_double,
                                 ctypes.c_uint64, vp, vp])}


def in_struct(member):
    return "#define T_MAX 3\ntypedef struct t_s {\n  int n;\n  %s\n} t_s;\n" % member


@pytest.mark.parametrize("text", [
    in_struct("unsigned n2;"),                        # an unknown base type
    in_struct("long n2;"),
    in_struct("t_unknown inner;"),                    # a struct nobody declared
    in_struct("const t_unknown* p;"),
    in_struct("int flag : 3;"),                       # a bit-field
    in_struct("int (*callback)(int);"),               # a function pointer
    in_struct("union { int i; float f; } u;"),        # a union
    in_struct("struct { int i; } anon;"),             # a nested anonymous struct
    in_struct("float thr[T_OTHER];"),                 # an array bound that is no known constant
    in_struct("float thr[T_MAX + 1];"),
    in_struct("float thr[0];"),
    in_struct("float** rows;"),
    in_struct("float *a, b;"),                        # one '*', two declarators
    "typedef struct t_s { int n; } t_other;",         # typedef name is not the tag
    "int t_f(unsigned n);",                           # prototypes: parameter and return types
    "int t_f(const t_unknown* args);",
    "int t_f(int);",
    "int t_f(int (*cb)(int));",
    "float* t_f(void);",
    "long t_f(void);",
    "typedef int t_int;",                             # file scope: anything else
    "static inline int t_f(void) { return 0; }",
    "enum t_kind { T_A = 1 << 2 };",
    "#pragma pack(push, 1)\ntypedef struct t_s { int n; } t_s;",
    "#if T_WIDE\ntypedef struct t_s { int n; } t_s;\n#endif",
    "int t_f(void)",                                  # an unterminated tail
])
def test_what_it_cannot_match_raises(tmp_path, text):
    with pytest.raises(cabi.HeaderError, match=r"t\.h"):
        parse_text(tmp_path, text)


def test_each_case_fails_for_its_own_member(tmp_path):
    """The frame of the struct cases is itself readable: only the member raises."""
    h = parse_text(tmp_path, in_struct("float thr[T_MAX];"))
    assert h.structs["t_s"]._fields_ == [("n", ctypes.c_int), ("thr", ctypes.c_float * 3)]
    with pytest.raises(cabi.HeaderError, match="flag : 3"):
        parse_text(tmp_path, in_struct("int flag : 3;"))
