"""CPU-only: super_primitive_amd/_lib.py is a hand-written mirror of include/sp_hip.h, and this file holds ALL of it to the header --
every prototype by argument and return type, every record field by field, every constant -- from one parse (tests/abi_header.py).
Each comparison returns what it found as a list of sentences, so that the last test can plant errors in copies of the tables and see
every one of them reported."""
import ctypes
import inspect
import re
from ctypes import c_double, c_float, c_int, c_longlong, c_void_p

import pytest

import abi_header
from super_primitive_amd import _lib

CLASS_OF = {c_void_p: abi_header.POINTER, c_int: "int", c_longlong: "long long", c_float: "float", c_double: "double"}
DEVICE_ONLY = {"SpRunDesc"}                 # records of the header that only kernels read and write: no ctypes mirror
ALIASES = {"inp": "in"}                     # mirror field name -> header field name (``in`` is a Python keyword)


@pytest.fixture(scope="module")
def header():
    return abi_header.parse()


def mirror_structs(module=_lib):
    return {name: cls for name, cls in vars(module).items() if isinstance(cls, type) and issubclass(cls, ctypes.Structure)}


def mirror_constants(module=_lib):
    return {name: v for name, v in vars(module).items() if name.startswith("SP_") and type(v) is int}


def status_failed_bits(source):
    """The names that the definition of SP_STATUS_FAILED in ``source`` ORs together."""
    return [s.strip() for s in re.search(r"^SP_STATUS_FAILED\s*=\s*(.+)$", source, flags=re.M).group(1).split("|")]


def derived_constants(defines, structs, source):
    """What the mirror's constants WITHOUT a define of their own must equal, each from what it derives from."""
    bits = status_failed_bits(source)
    assert len(bits) > 1 and all(b.startswith("SP_STATUS_") and b in defines for b in bits), bits
    failed = 0
    for b in bits:
        failed |= defines[b]
    return {"SP_VIEW_FLOATS": structs["SpView"]["size"] / 4, "SP_TRAJ_ALIGN_DOUBLES": structs["SpTrajAlign"]["size"] / 8,
            "SP_STATUS_FAILED": failed}


def signature_errors(prototypes, signatures, restypes):
    errors = [f"{name}: a signature with no prototype" for name in sorted(set(signatures) - set(prototypes))]
    errors += [f"{name}: a prototype with no signature" for name in sorted(set(prototypes) - set(signatures))]
    errors += [f"{name}: a restype with no signature" for name in sorted(set(restypes) - set(signatures))]
    for name in sorted(set(signatures) & set(prototypes)):
        ret, args, names = prototypes[name]
        mine = [CLASS_OF.get(a, repr(a)) for a in signatures[name]]
        if len(mine) != len(args):
            errors.append(f"{name}: {len(mine)} arguments, the header has {len(args)}")
        errors += [f"{name}: argument {i} ({names[i]}) is {m}, the header says {a}" for i, (m, a) in enumerate(zip(mine, args)) if m != a]
        res = CLASS_OF.get(restypes.get(name, c_int), repr(restypes.get(name)))
        if res != ret:
            errors.append(f"{name}: returns {res}, the header says {ret}")
    return errors


def struct_errors(structs, mirrors, device_only=DEVICE_ONLY):
    errors = [f"{name}: a ctypes record with no struct in the header" for name in sorted(set(mirrors) - set(structs))]
    errors += [f"{name}: listed as device-only and mirrored" for name in sorted(device_only & set(mirrors))]
    for name, rec in structs.items():
        if rec["stated"] != rec["size"]:
            errors.append(f"{name}: SP_ABI_SIZE states {rec['stated']}, the fields lay out to {rec['size']}")
        if name not in mirrors:
            if name not in device_only:
                errors.append(f"{name}: a struct of the header with no ctypes record")
            continue
        cls = mirrors[name]
        mine = [(ALIASES.get(f[0], f[0]), getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
        if ctypes.sizeof(cls) != rec["size"]:
            errors.append(f"{name}: {ctypes.sizeof(cls)} bytes, the header has {rec['size']}")
        if len(mine) != len(rec["fields"]):
            errors.append(f"{name}: {len(mine)} fields, the header has {len(rec['fields'])}")
        errors += [f"{name}: field {i} is (name, offset, size) = {m}, the header has {h}" for i, (m, h) in enumerate(zip(mine, rec["fields"]))
                   if m != h]
    return errors


def constant_errors(defines, constants, derived):
    errors = []
    for name, value in sorted(constants.items()):
        if name not in derived and name not in defines:
            errors.append(f"{name}: neither a #define of the header nor a derived value")
        elif value != derived.get(name, defines.get(name)):
            errors.append(f"{name}: {value}, the header gives {derived.get(name, defines.get(name))}")
    return errors + [f"{name}: derived and defined" for name in sorted(set(derived) & set(defines))]


def test_every_prototype_matches_the_signature_table_and_the_loaded_library(header):
    prototypes = header[0]
    assert len(prototypes) > 90
    assert signature_errors(prototypes, _lib.SIGNATURES, _lib.RESTYPES) == []
    lib = _lib.load()
    for name, (ret, args, _) in prototypes.items():
        fn = getattr(lib, name)
        assert [CLASS_OF[a] for a in fn.argtypes] == args and list(fn.argtypes) == _lib.SIGNATURES[name], name
        assert CLASS_OF[fn.restype] == ret and fn.restype is _lib.RESTYPES.get(name, c_int), name
    # the stream a launch goes to is the last parameter, and nothing else is called `stream`
    for name, (_, args, names) in prototypes.items():
        assert "stream" not in names[:-1] and (names[-1:] != ["stream"] or args[-1] == abi_header.POINTER), name


def test_every_struct_matches_its_ctypes_record_field_by_field(header):
    structs = header[2]
    assert len(structs) > 20 and DEVICE_ONLY <= set(structs)
    assert struct_errors(structs, mirror_structs()) == []


def test_every_constant_matches_its_define(header):
    _, defines, structs = header
    constants = mirror_constants()
    assert len(constants) > 50 and defines["SP_ABI_VERSION"] == 20
    assert constant_errors(defines, constants, derived_constants(defines, structs, inspect.getsource(_lib))) == []


def test_the_parser_refuses_what_it_cannot_classify(tmp_path):
    for text, complaint in (("int sp_f(unsigned n);", "parameter n"), ("short sp_f(int n);", "return value"), ("int sp_f(int);", "parameter 0"),
                            ("typedef struct { size_t n; } SpX;", "unknown type"), ("typedef struct { int n[SP_N]; } SpX;", "dimension"),
                            ("typedef struct { int n; } SpX;\nSP_ABI_SIZE(SpY, 4)", "SP_ABI_SIZE")):
        (tmp_path / "h.h").write_text(text)
        with pytest.raises(ValueError, match=complaint):
            abi_header.parse(str(tmp_path / "h.h"))
    (tmp_path / "h.h").write_text("#define SP_A 3\n#define SP_B (SP_A | 1LL << 4) /* c */\n#define SP_F 1.5e-3\n#define SP_M(k) (k)\n"
                                  "typedef struct SpX { char c; double d[SP_A], *p; struct SpX* q; } SpX;\nSP_ABI_SIZE(SpX, 48)\n"
                                  "typedef struct { SpX x[2]; int32_t n; } SpY;\nlong long sp_f(const struct SpX* const* x, double d);")
    prototypes, defines, structs = abi_header.parse(str(tmp_path / "h.h"))
    assert prototypes == {"sp_f": ("long long", ["pointer", "double"], ["x", "d"])} and defines == {"SP_A": 3, "SP_B": 19}
    assert structs["SpX"] == {"fields": [("c", 0, 1), ("d", 8, 24), ("p", 32, 8), ("q", 40, 8)], "size": 48, "align": 8, "stated": 48}
    assert structs["SpY"] == {"fields": [("x", 0, 96), ("n", 96, 4)], "size": 104, "align": 8, "stated": None}


def test_planted_errors_are_reported_by_name(header):
    prototypes, defines, structs = header

    def signatures(**changed):
        return {**{k: list(v) for k, v in _lib.SIGNATURES.items()}, **changed}

    def argument(name, cls, becomes):
        """``name``'s list with its first argument of ctypes class ``cls`` replaced."""
        args = list(_lib.SIGNATURES[name])
        at = args.index(cls)
        args[at] = becomes
        return at, args

    at, args = argument("sp_pack_rgb", c_int, c_float)
    assert signature_errors(prototypes, signatures(sp_pack_rgb=args), _lib.RESTYPES) == [
        f"sp_pack_rgb: argument {at} (B) is float, the header says int"]
    at, args = argument("sp_map_fuse", c_longlong, c_int)
    assert signature_errors(prototypes, signatures(sp_map_fuse=args), _lib.RESTYPES) == [
        f"sp_map_fuse: argument {at} (Q) is int, the header says long long"]
    assert signature_errors(prototypes, signatures(), {"sp_tsdf_mesh_scratch_bytes": c_int}) == [
        "sp_tsdf_mesh_scratch_bytes: returns int, the header says long long"]
    assert signature_errors(prototypes, signatures(), {}) == ["sp_tsdf_mesh_scratch_bytes: returns int, the header says long long"]
    assert signature_errors(prototypes, signatures(sp_pairs_cost_active=[c_void_p]), _lib.RESTYPES) == [
        "sp_pairs_cost_active: a signature with no prototype"]
    assert signature_errors(prototypes, signatures(sp_pack_rgb=_lib.SIGNATURES["sp_pack_rgb"][:-1]), _lib.RESTYPES) == [
        "sp_pack_rgb: 5 arguments, the header has 6"]

    def record(name, fields):
        return {**mirror_structs(), name: type(name, (ctypes.Structure,), {"_fields_": fields})}

    fields = list(_lib.SpPhase._fields_)
    at = [f[0] for f in fields].index("n_spans")
    assert [f[0] for f in fields[at:at + 2]] == ["n_spans", "max_iters"] and fields[at][1] is fields[at + 1][1]
    fields[at], fields[at + 1] = fields[at + 1], fields[at]
    assert struct_errors(structs, record("SpPhase", fields)) == [
        f"SpPhase: field {at} is (name, offset, size) = ('max_iters', 40, 4), the header has ('n_spans', 40, 4)",
        f"SpPhase: field {at + 1} is (name, offset, size) = ('n_spans', 44, 4), the header has ('max_iters', 44, 4)"]
    short = record("SpWindowBlock", _lib.SpWindowBlock._fields_[:-1])          # the last float gone: padding keeps the size
    assert ctypes.sizeof(short["SpWindowBlock"]) == ctypes.sizeof(_lib.SpWindowBlock)
    assert struct_errors(structs, short) == ["SpWindowBlock: 4 fields, the header has 5"]
    assert struct_errors(structs, {k: v for k, v in mirror_structs().items() if k != "SpView"}) == [
        "SpView: a struct of the header with no ctypes record"]
    restated = {**structs, "SpView": {**structs["SpView"], "stated": 104}}
    assert struct_errors(restated, mirror_structs()) == ["SpView: SP_ABI_SIZE states 104, the fields lay out to 100"]

    source = inspect.getsource(_lib)
    derived = derived_constants(defines, structs, source)
    assert constant_errors(defines, {**mirror_constants(), "SP_MAX_PHASES": _lib.SP_MAX_PHASES + 1}, derived) == [
        f"SP_MAX_PHASES: {_lib.SP_MAX_PHASES + 1}, the header gives {_lib.SP_MAX_PHASES}"]
    assert constant_errors(defines, {**mirror_constants(), "SP_VIEW_FLOATS": 26}, derived) == ["SP_VIEW_FLOATS: 26, the header gives 25.0"]
    assert constant_errors(defines, {**mirror_constants(), "SP_NEW_LIMIT": 7}, derived) == [
        "SP_NEW_LIMIT: neither a #define of the header nor a derived value"]
    fewer = derived_constants(defines, structs, source.replace("SP_STATUS_NONFINITE | ", "", 1))
    assert constant_errors(defines, mirror_constants(), fewer) == [
        f"SP_STATUS_FAILED: {_lib.SP_STATUS_FAILED}, the header gives {_lib.SP_STATUS_FAILED & ~_lib.SP_STATUS_NONFINITE}"]
