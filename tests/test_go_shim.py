"""shim/go/ holds the cgo binding a maintainer of the reference adds.  No Go toolchain exists in this image, so the
files cannot be compiled here; what CAN be checked is that they and the C ABI have not drifted apart: every C function, constant and
record the Go files name exists in include/bowgpu.h, the kind tags equal the header's enum values, and call sites pass the number of
arguments the prototypes take."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
GO = {f: open(f).read() for f in glob.glob(os.path.join(ROOT, "shim", "go", "**", "*.go"), recursive=True)}


def _enums():
    vals = {}
    for body in re.findall(r"enum\s*\{(.*?)\};", HDR, flags=re.S):
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        nxt = 0
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            m = re.match(r"(\w+)\s*(?:=\s*(-?\d+))?$", item)
            assert m, item
            nxt = int(m.group(2)) if m.group(2) is not None else nxt
            vals[m.group(1)] = nxt
            nxt += 1
    for m in re.finditer(r"#define\s+(BOWGPU_\w+)\s+(-?\d+)", HDR):
        vals[m.group(1)] = int(m.group(2))
    return vals


def _prototypes():
    flat = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int|const char \*)\s*(bowgpu_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_shim_files_exist_and_are_go_shaped():
    names = {os.path.relpath(f, os.path.join(ROOT, "shim", "go")) for f in GO}
    assert {"bowfill_gpu.go", "bowfill_gpu_off.go", "rolling/gpu_cgo.go", "rolling/gpu_off.go", "rolling/gpu_kinds.go", "rolling/transformation/gpu_factor.go",
            "rolling/aggregation/whole_gpu.go"} <= names
    # (round 3 shipped two comment-only files for the constructors: they are real diffs now, shim/go/patches/0002, 0003)
    assert not {"rolling/aggregation/gpu_kinds.go", "rolling/interpolation/gpu_kinds.go"} & names
    for f, src in GO.items():
        assert re.search(r"^package \w+$", src, flags=re.M), f
        code = re.sub(r"//.*", "", src)
        assert code.count("{") == code.count("}") and code.count("(") == code.count(")"), f
        assert "\t" in src or "gpu_kinds.go" in f, f        # gofmt indents with tabs


def test_every_c_name_the_shim_uses_is_in_the_header():
    enums, protos = _enums(), _prototypes()
    structs = set(re.findall(r"typedef struct (bowgpu_\w+)", HDR))
    used_fn, used_const = set(), set()
    for f, src in GO.items():
        code = re.sub(r"//.*", "", src)
        for name in re.findall(r"\bC\.(bowgpu_\w+)\s*\(", code):
            used_fn.add(name)
        for name in re.findall(r"\bC\.(BOWGPU_\w+)", code):
            used_const.add(name)
        for name in re.findall(r"\bC\.sizeof_(bowgpu_\w+)", code):
            assert name in structs, (f, name)
        for name in re.findall(r"\bC\.(bowgpu_\w+)\b(?!\s*\()", code):
            assert name in structs or name in protos, (f, name)
    assert used_fn and used_fn <= set(protos), used_fn - set(protos)
    assert used_const <= set(enums), used_const - set(enums)
    # the entry points of the hot path are bound
    assert {"bowgpu_rolling_aggregate", "bowgpu_abi_version", "bowgpu_rolling_interpolate_count", "bowgpu_rolling_interpolate_fill",
            "bowgpu_fill_linear_sorted", "bowgpu_fill", "bowgpu_is_col_sorted", "bowgpu_set_devices", "bowgpu_device_count",
            "bowgpu_host_register", "bowgpu_host_unregister", "bowgpu_last_error", "bowgpu_aggregate_whole"} <= used_fn


def test_call_sites_pass_as_many_arguments_as_the_prototypes_take():
    protos = _prototypes()
    for f, src in GO.items():
        code = re.sub(r"//.*", "", src)
        for m in re.finditer(r"\bC\.(bowgpu_\w+)\s*\(", code):
            depth, i, args, cur = 1, m.end(), 0, ""
            while depth:
                ch = code[i]
                depth += ch in "([{"
                depth -= ch in ")]}"
                if ch == "," and depth == 1:
                    args += 1
                elif depth:
                    cur += ch
                i += 1
            n = 0 if not cur.strip() and args == 0 else args + 1
            assert n == protos[m.group(1)], (os.path.basename(f), m.group(1), n, protos[m.group(1)])


def test_kind_tags_equal_the_header_enums():
    enums = _enums()
    kinds = GO[os.path.join(ROOT, "shim", "go", "rolling", "gpu_kinds.go")]
    got = {k: int(v) for k, v in re.findall(r"\b(GPU\w+)\s+int32\s*=\s*(-?\d+)", kinds)}
    want = {"GPUKindWindowStart": "BOWGPU_AGG_WINDOW_START", "GPUKindSum": "BOWGPU_AGG_SUM", "GPUKindArithmeticMean": "BOWGPU_AGG_MEAN",
            "GPUKindMin": "BOWGPU_AGG_MIN", "GPUKindMax": "BOWGPU_AGG_MAX", "GPUKindCount": "BOWGPU_AGG_COUNT", "GPUKindFirst": "BOWGPU_AGG_FIRST",
            "GPUKindLast": "BOWGPU_AGG_LAST", "GPUKindIntegralStep": "BOWGPU_AGG_INTEGRAL_STEP",
            "GPUKindIntegralTrapezoid": "BOWGPU_AGG_INTEGRAL_TRAPEZOID", "GPUKindWeightedAvgStep": "BOWGPU_AGG_WAVG_STEP",
            "GPUKindWeightedAvgLinear": "BOWGPU_AGG_WAVG_LINEAR", "GPUKindMode": "BOWGPU_AGG_MODE",
            "GPUInterpWindowStart": "BOWGPU_INTERP_WINDOW_START", "GPUInterpLinear": "BOWGPU_INTERP_LINEAR",
            "GPUInterpStepPrevious": "BOWGPU_INTERP_STEP_PREVIOUS", "GPUInterpNone": "BOWGPU_INTERP_NONE"}
    for g, h in want.items():
        assert got[g] == enums[h], (g, got[g], h, enums[h])
    assert got["GPUKindNone"] == -1
    # bow.Type values the shim passes through as bowgpu_col.type (bowtypes.go:21-23)
    assert enums["BOWGPU_FLOAT64"] == 1 and enums["BOWGPU_INT64"] == 2


# ---------------------------------------------------------------- the shim against the REFERENCE's types
# tests/golden/go_type_shapes.json: struct fields / method sets of the reference types the shim reads or extends, extracted from
# /root/reference by shim/go/make_patches.py in the build container (the reference itself never travels to the GPU box).
import json
import shutil
import subprocess
import sys

SHAPES = json.load(open(os.path.join(ROOT, "tests", "golden", "go_type_shapes.json")))
PATCH_DIR = os.path.join(ROOT, "shim", "go", "patches")
PATCHES = {f: open(os.path.join(PATCH_DIR, f)).read() for f in sorted(os.listdir(PATCH_DIR)) if f.endswith(".patch")}
REF = os.environ.get("BOW_REFERENCE", "/root/reference")


def _go(rel):
    return re.sub(r"//.*", "", GO[os.path.join(ROOT, "shim", "go", *rel.split("/"))])


def _added_by_patches(rel):
    """lines the patches add to one reference file"""
    out, cur = [], None
    for text in PATCHES.values():
        for line in text.split("\n"):
            if line.startswith("+++ b/"):
                cur = line[6:]
            elif cur == rel and line.startswith("+") and not line.startswith("+++"):
                out.append(line[1:])
    return "\n".join(out)


def test_the_tag_is_a_field_of_the_reference_types_not_a_wrapper():
    """ColInterpolation is a struct (no type assertion on it, no embedding wrapper returned as one), and a
    wrapper around the ColAggregation interface loses its tag in RenameOutput / SetTransformations, which copy the inner struct."""
    assert SHAPES["rolling.ColInterpolation"]["kind"] == "struct" and SHAPES["rolling.ColAggregation"]["kind"] == "interface"
    assert {"RenameOutput", "SetTransformations"} <= set(SHAPES["rolling.colAggregation"]["methods"])   # the copying methods live on the struct
    every = "\n".join(_go(os.path.relpath(f, os.path.join(ROOT, "shim", "go"))) for f in GO)
    assert "kindedAggregation" not in every and "kindedInterpolation" not in every and "gpuKinded" not in every
    assert not re.search(r"\bip\.\(", every)                      # no type assertion on a ColInterpolation value
    # the field is added to BOTH structs by patch 0001, and only there
    assert re.search(r"^\tgpuKind int32", _added_by_patches("rolling/aggregation.go"), flags=re.M)
    assert re.search(r"^\tgpuKind int32", _added_by_patches("rolling/interpolation.go"), flags=re.M)
    assert "gpuKind" not in SHAPES["rolling.colAggregation"]["fields"] + SHAPES["rolling.ColInterpolation"]["fields"]
    kinds = _go("rolling/gpu_kinds.go")
    assert re.search(r"NewColAggregation\(inputName, needInclusiveWindow, typ, fn\)\.\(\*colAggregation\)", kinds)   # the concrete type NewColAggregation returns
    assert "a.gpuKind = kind + 1" in kinds and "ip.gpuKind = kind + 1" in kinds
    # runtime.Pinner needs Go 1.21: stated as a build constraint, with a fallback file for everything else
    assert "//go:build bowgpu && go1.21" in GO[os.path.join(ROOT, "shim", "go", "rolling", "gpu_cgo.go")]
    assert "//go:build !(bowgpu && go1.21)" in GO[os.path.join(ROOT, "shim", "go", "rolling", "gpu_off.go")]
    assert SHAPES["go.mod"]["go"] == "1.18"


def test_every_identifier_the_shim_uses_on_a_reference_type_exists_there():
    cgo, kinds, off = _go("rolling/gpu_cgo.go"), _go("rolling/gpu_kinds.go"), _go("rolling/gpu_off.go")
    R = SHAPES["rolling.intervalRolling"]
    lazy = _go("rolling/gpu_lazy.go")
    shim_methods = set(re.findall(r"^func \(r \*intervalRolling\) (\w+)\(", cgo + lazy, flags=re.M))
    assert shim_methods - set(R["methods"]) == shim_methods        # the shim adds methods, it does not redefine the reference's
    assert set(re.findall(r"^func \(r \*intervalRolling\) (\w+)\(", off, flags=re.M)) == {"aggregateWindowsGPU", "interpolateWindowsGPU", "lazyInterpolationGPU",
                                                                                       "interpolateAggregateGPU"} <= shim_methods
    for name in set(re.findall(r"\b(?:r|rCopy)\.(\w+)", lazy)):
        assert name in R["fields"] or name in R["methods"] or name in shim_methods, ("intervalRolling", name)
    # the lazy Rolling implements the whole Rolling interface (rolling.go:14-29) and nothing else the reference does not know
    assert sorted(set(re.findall(r"^func \(l \*lazyInterpolation\) (\w+)\(", lazy, flags=re.M)) - {"materialised"}) == SHAPES["rolling.Rolling"]["methods"]
    assert "rCopy.lazyInterpolationGPU(interps, newIntervalCol); lazy != nil" in _added_by_patches("rolling/interpolation.go")
    for fn in ("intervalRolling.interpolateWindows", "newIntervalRolling"):
        want = SHAPES["error_strings"]["rolling/interpolation.go wraps %s" % fn]     # the reference's own wording of the wrap
        assert want == fn + ": %w" and 'fmt.Errorf("%s", err)' % want in lazy
    for name in set(re.findall(r"\br\.(\w+)", cgo)):
        assert name in R["fields"] or name in R["methods"] or name in shim_methods, ("intervalRolling", name)
    for name in set(re.findall(r"\br\.options\.(\w+)", cgo)):
        assert name in SHAPES["rolling.Options"]["fields"], ("Options", name)
    bow_methods = set(SHAPES["bow.Bow"]["methods"])
    for name in set(re.findall(r"\b(?:r\.bow|pr|b)\.(\w+)\(", cgo)):
        assert name in bow_methods, ("bow.Bow", name)
    for name in set(re.findall(r"\bbow\.(New\w+)\(", cgo)):
        assert name in SHAPES["bow.funcs"]["funcs"], ("package bow", name)
    agg_methods = set(SHAPES["rolling.ColAggregation"]["methods"])
    for name in set(re.findall(r"\ba\.(\w+)\(", cgo)):
        assert name in agg_methods, ("ColAggregation", name)
    for name in set(re.findall(r"\bip\.(\w+)", cgo + kinds)):
        assert name in SHAPES["rolling.ColInterpolation"]["fields"] + ["gpuKind"], ("ColInterpolation", name)
    for name in set(re.findall(r"\b(?:ca|a)\.(\w+)\b(?!\()", kinds)):
        assert name in SHAPES["rolling.colAggregation"]["fields"] + ["gpuKind"], ("colAggregation", name)
    for name in ("NewColAggregation", "NewColInterpolation"):
        assert name in SHAPES["rolling.funcs"]["funcs"]
    # transformation.Func is a func type: a Factor is recognised by its code pointer, not by an interface it cannot implement
    assert SHAPES["transformation"]["Func"].startswith("func(interface{})") and "Factor" in SHAPES["transformation"]["funcs"]
    fac = _go("rolling/transformation/gpu_factor.go")
    assert "func FactorOf(f Func) (n float64, ok bool)" in fac and "reflect.ValueOf(Factor(1)).Pointer()" in fac
    assert "transformation.FactorOf(t)" in cgo and "gpuKindOfAggregation(a)" in cgo
    # the hooks call what both build variants define, and compare with the sentinel both define
    hooks = _added_by_patches("rolling/aggregation.go") + _added_by_patches("rolling/interpolation.go")
    assert "r.aggregateWindowsGPU(aggrs); err != errDeclined" in hooks and "r.interpolateWindowsGPU(interps); err != errDeclined" in hooks
    assert "var errDeclined" in cgo and "var errDeclined" in off


def test_every_builtin_constructor_is_tagged_by_the_patches():
    kinds = _go("rolling/gpu_kinds.go")
    tags = set(re.findall(r"\b(GPU(?:Kind|Interp)\w+)\s+int32", kinds)) - {"GPUKindNone"}
    used = set(re.findall(r"rolling\.(GPU(?:Kind|Interp)\w+)", "\n".join(PATCHES.values())))
    assert used == tags, (tags - used, used - tags)
    for text in (PATCHES["0002-aggregation-constructors-carry-their-kind.patch"], PATCHES["0003-interpolation-constructors-carry-their-kind.patch"]):
        minus = [l for l in text.split("\n") if l.startswith("-") and not l.startswith("---")]
        plus = [l for l in text.split("\n") if l.startswith("+") and not l.startswith("+++")]
        assert all("rolling.NewCol" in l or l.strip("-\t ") in ("})", ")") for l in minus), minus
        assert all("GPU" in l for l in plus), plus              # nothing but the constructor name and the tag changes: the closures are untouched


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")
def test_patches_are_reproduced_from_the_reference_and_apply_cleanly(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "shim", "go", "make_patches.py"), "--check"])
    touched = sorted({l[6:] for t in PATCHES.values() for l in t.split("\n") if l.startswith("+++ b/")})
    for rel in touched:
        os.makedirs(os.path.dirname(tmp_path / rel), exist_ok=True)
        shutil.copy(os.path.join(REF, rel), tmp_path / rel)
    for name in PATCHES:
        subprocess.check_call(["patch", "-p1", "-s", "-i", os.path.join(PATCH_DIR, name)], cwd=tmp_path)
    agg = open(tmp_path / "rolling/aggregation.go").read()
    assert agg.count("gpuKind int32") == 1 and "aCopy := *a" in agg                       # the copy keeps the new field
    assert "rolling.NewColAggregationGPU(col, false, bow.Float64," in open(tmp_path / "rolling/aggregation/arithmeticmean.go").read()
    for rel in touched:
        code = re.sub(r"//.*", "", open(tmp_path / rel).read())
        assert code.count("{") == code.count("}") and code.count("(") == code.count(")"), rel


# ---------------------------------------------------------------- round 5: no dead binding, the reference's error texts
def _patched_and_shim_sources():
    """every line the patches ADD to the reference plus every shim file: the code that exists only because of the shim"""
    added = "\n".join(l[1:] for t in PATCHES.values() for l in t.split("\n") if l.startswith("+") and not l.startswith("+++"))
    return added, {os.path.relpath(f, os.path.join(ROOT, "shim", "go")): re.sub(r"//.*", "", src) for f, src in GO.items()}


def test_every_gpu_function_the_shim_defines_has_a_caller():
    """fillLinearGPU / fillGPU / isColSortedGPU were defined and nothing called them - no patch touched bowfill.go or
    bowassertion.go - and aggregation.Aggregate had no binding at all.  Every `...GPU` function or method a shim file defines must be
    called from a line some patch adds to the reference or from another shim file; the one stated exception is the application's own
    entry point RegisterForGPU.  (Round 6: aggregateShardGPU - a rank of the shard protocol for an application-side transport, never
    called - is gone: the library spreads ONE Aggregate call over the devices itself, bowgpu_set_devices, which init() switches on
    through SetGPUDevices.)"""
    added, files = _patched_and_shim_sources()
    defined = {}
    for rel, code in files.items():
        for m in re.finditer(r"^func (?:\(\w+ \*?\w+\) )?(\w*GPU\w*)\(", code, flags=re.M):
            defined.setdefault(m.group(1), set()).add(rel)
    assert {"fillLinearGPU", "fillGPU", "isColSortedGPU", "aggregateWholeGPU", "AggregateWholeGPU", "aggregateWindowsGPU", "interpolateWindowsGPU",
            "NewColAggregationGPU", "NewColInterpolationGPU"} <= set(defined)
    entry_points = {"RegisterForGPU"}
    assert "aggregateShardGPU" not in defined and "SetGPUDevices" in defined
    cgo = files["rolling/gpu_cgo.go"]
    assert "C.bowgpu_set_devices(&c[0], C.int(len(c)))" in cgo and "_ = SetGPUDevices(ids)" in cgo[cgo.index("func init()"):cgo.index("func SetGPUDevices")]
    for name, where in defined.items():
        calls = len(re.findall(r"(?<!func )(?<!\) )\b%s\(" % name, added))
        for rel, code in files.items():
            body = re.sub(r"^func (?:\(\w+ \*?\w+\) )?%s\(" % name, "", code, flags=re.M)    # its own definition is not a call
            calls += len(re.findall(r"\b%s\(" % name, body))
        assert calls > 0 or name in entry_points, "%s (defined in %s) has no caller in the patched tree" % (name, sorted(where))
    # the hooks sit in the functions VERDICT names, behind the reference's own argument checks
    fill = _added_by_patches("bowfill.go")
    assert "b.fillLinearGPU(refColIndex, toFillColIndex); err != errGPUDeclined" in fill and fill.count("b.fillGPU(colIndex, ") == 2
    assert 'b.fillGPU(colIndex, "Mean")' in fill and "b.fillGPU(colIndex, method)" in fill
    assert "b.isColSortedGPU(colIndex); err != errGPUDeclined" in _added_by_patches("bowassertion.go")
    assert "aggregateWholeGPU(b, intervalColIndex, aggrs); err != rolling.ErrGPUDeclined" in _added_by_patches("rolling/aggregation/whole.go")
    # both build variants define what the hooks call and compare with
    on, off = files["bowfill_gpu.go"], files["bowfill_gpu_off.go"]
    for sym in ("var errGPUDeclined", "func (b *bow) fillLinearGPU(refCol, toFillCol int) (Bow, error)", "func (b *bow) fillGPU(colIndex int, method string) (Series, bool)",
                "func (b *bow) isColSortedGPU(colIndex int) (bool, error)", "func RegisterForGPU(b Bow) (release func())",
                "func GPUResidency(values, validity unsafe.Pointer) int32"):
        assert sym in on and sym in off, sym
    assert "//go:build bowgpu && go1.21" in GO[os.path.join(ROOT, "shim", "go", "bowfill_gpu.go")]
    assert "//go:build !(bowgpu && go1.21)" in GO[os.path.join(ROOT, "shim", "go", "bowfill_gpu_off.go")]
    ron, roff = files["rolling/gpu_cgo.go"], files["rolling/gpu_off.go"]
    for sym in ("var ErrGPUDeclined = errDeclined", "func AggregateWholeGPU(b bow.Bow, intervalColIndex int, aggrs []ColAggregation) (bow.Bow, error)",
                "func RegisterForGPU(b bow.Bow) (release func())", "func SetGPUDevices(ids []int) error"):
        assert sym in ron and sym in roff, sym


def test_the_error_texts_the_shim_words_are_the_references():
    """bowfill.go:40-41 says "refColIndex '%d' is empty or not sorted"; round 4's binding said "bow.FillLinear: column '%s' is ..."."""
    texts = SHAPES["error_strings"]
    fill = GO[os.path.join(ROOT, "shim", "go", "bowfill_gpu.go")]
    cgo = GO[os.path.join(ROOT, "shim", "go", "rolling", "gpu_cgo.go")]
    want = texts["bowfill.go FillLinear not sorted"]
    assert want == "refColIndex '%d' is empty or not sorted"
    assert 'fmt.Errorf("%s", refCol)' % want in fill
    assert 'fmt.Errorf("%s", intervalCol)' % texts["rolling/aggregation.go keep interval"] in cgo
    # every other fmt.Errorf / errors.New text in the bow-package binding is the decline sentinel's own
    worded = set(re.findall(r'(?:fmt\.Errorf|errors\.New)\("([^"]*)"', re.sub(r"//.*", "", fill)))
    assert worded == {want, "bowgpu: input outside the device path"}, worded


def test_registered_buffers_reach_the_library_as_pinned_residency():
    """RegisterForGPU existed but colDesc always passed BOWGPU_HOST - the zero-copy residency was unreachable from Go"""
    fill, cgo = _go("bowfill_gpu.go"), _go("rolling/gpu_cgo.go")
    assert "gpuRegistered.Store(p, buf.Len())" in fill and "C.bowgpu_host_register(p, C.int64_t(buf.Len()))" in fill
    assert "return int32(C.BOWGPU_HOST_PINNED)" in fill
    assert "c.residency = C.int32_t(GPUResidency(c.values, unsafe.Pointer(c.validity)))" in fill
    assert "c.residency = C.int32_t(bow.GPUResidency(c.values, unsafe.Pointer(c.validity)))" in cgo
    assert "c.residency = C.BOWGPU_HOST" not in cgo and "c.residency = C.BOWGPU_HOST" not in fill.replace("C.BOWGPU_HOST_PINNED", "")


def test_the_bow_package_binding_uses_only_what_the_reference_defines():
    code = _go("bowfill_gpu.go")
    B = SHAPES["bow.bow"]
    assert B["fields"] == ["arrow.Record"]
    record_methods = {"ColumnName", "Column", "Schema", "NumCols", "NumRows"}     # arrow.Record, through the embedded field
    for name in set(re.findall(r"\bb\.(\w+)\(", code)):
        assert name in B["methods"] or name in record_methods or name.endswith("GPU"), ("bow", name)
    for name in set(re.findall(r"(?<![.\w])(New\w+)\(", code)):
        assert name in SHAPES["bow.funcs"]["funcs"], ("package bow", name)
    whole = _go("rolling/aggregation/whole_gpu.go")
    for name in set(re.findall(r"\baggr\.(\w+)\(", whole)):
        assert name in SHAPES["rolling.ColAggregation"]["methods"], ("ColAggregation", name)
    for name in set(re.findall(r"\bb\.(\w+)\(", whole)):
        assert name in SHAPES["bow.Bow"]["methods"], ("bow.Bow", name)
