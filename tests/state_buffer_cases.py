"""The refused calls of the rasteriser's entry points that take a state buffer, shared by tests/test_abi.py
(test_state_buffer_refusals_are_the_recorded_ones) and tools/record_state_buffer_refusals.py, which wrote tests/golden/state_buffer_refusals.json.

One call per (entry point, pointer argument, fault): the buffer NULL, the buffer one byte shorter than its *_bytes function reports, or one of
the entry point's other pointers (radii, grads, dL_*, out_*, ...) NULL -- every other argument acceptable: a dummy host address for the
pointers, P = 100, D = 10, a 64x96 frame, precomputed colours in three channels, three classes, a huge size for the buffers not under test.
Only refused calls are made, and every refusal here comes before the entry point's first HIP call (AFTER_A_HIP_CALL: the one that does
not), so nothing needs a GPU.
"""
import ctypes

from streetunveiler_amd import _lib

P, D, H, W, N_CLASSES, BIG = 100, 10, 64, 96, 3, 1 << 40

# entry point -> its arguments in the header's order (without the closing stream).  A buffer's name stands for (address, bytes); "@name" is
# another pointer; everything else is a value of the fixed scene.
ARGUMENTS = {
    "sr_geom_view": ["geom", "P", "@out"],
    "sr_binning_view": ["binning", "P", "D", "W", "H", "@out"],
    "sr_image_view": ["image", "W", "H", "@out"],
    "sr_forward_plan": ["frame", "g", "geom", "@radii", "@num_rendered_host"],
    "sr_forward_render": ["frame", "g", "geom", "binning", "image", "D", "@out_color", "@out_allmap"],
    "sr_backward_blend": ["frame", "g", "geom", "binning", "image", "D", "@dL_dcolor", "@dL_dallmap", "workspace"],
    "sr_backward_geometry": ["frame", "g", "@radii", "geom", "binning", "image", "D", "workspace", "@grads"],
    "sr_backward": ["frame", "g", "@radii", "geom", "binning", "image", "D", "@dL_dcolor", "@dL_dallmap", "workspace", "@grads"],
    "sr_backward_colors": ["frame", "g", "@radii", "geom", "D", "workspace", "@dL_dcolors"],
    "sr_class_forward_render": ["frame", "g", "n_classes", "geom", "binning", "class_image", "D", "@out_dist"],
    "sr_class_backward": ["frame", "g", "n_classes", "@radii", "geom", "binning", "class_image", "D", "@dL_ddist", "workspace", "@grads"],
    "sr_class_forward_shared": ["frame", "g", "n_classes", "@classes", "geom", "binning", "class_state", "D", "@out_dist"],
    "sr_class_backward_shared": ["frame", "g", "n_classes", "geom", "binning", "class_state", "D", "@dL_ddist", "workspace"],
    "sr_debug_pair_decisions": ["frame", "g", "geom", "binning", "D", "@valid_bits", "@use3d_bits"],
}
BUFFERS = ("geom", "binning", "image", "class_image", "class_state", "workspace")
VIEWS = {"sr_geom_view": _lib.SrGeomView, "sr_binning_view": _lib.SrBinningView, "sr_image_view": _lib.SrImageView}


def buffers_of(entry):
    return [a for a in ARGUMENTS[entry] if a in BUFFERS]


def pointers_of(entry):
    return [a[1:] for a in ARGUMENTS[entry] if a.startswith("@")]


# Refused only after a HIP call, so not in the table: sr_backward runs the whole of sr_backward_blend before sr_backward_geometry looks at
# radii (sr_backward_geometry's own row holds that refusal).
AFTER_A_HIP_CALL = {("sr_backward", "radii", "null")}


# A row's "case": what differs from the fixed scene (None: nothing) -- the number of duplicates, the number of Gaussians, the frame's flags.
# In all of them the forward kernel of sr_forward_render is the one the device picks per frame (16x16 tile, three channels; the one-wave
# backward does not change the forward kernel).
NO_DUPLICATES, NO_GAUSSIANS, NO_DUPLICATES_ONE_WAVE = "D = 0", "P = 0", "D = 0, SR_FLAG_ONE_WAVE_BACKWARD"
CASES = {None: {}, NO_DUPLICATES: {"D": 0}, NO_GAUSSIANS: {"P": 0, "D": 0}, NO_DUPLICATES_ONE_WAVE: {"D": 0, "flags": _lib.SR_FLAG_ONE_WAVE_BACKWARD}}
# Rows beyond faults(): (entry, argument, fault, case, also) -- `also`: a second fault in the same call, as ((argument, fault),).
# No recorded value ("recorded_text" null; the text was written into the table by hand): where there is nothing to bin the library the
# table was recorded from did not look at the geometry buffer and went on to its first launch -- in sr_forward_render with a frame-count
# pointer formed from a NULL one, in sr_class_forward_render staging P class bytes in one of any size.  Now a NULL one is refused where the
# device-picked kernel would read it (include/surfel_raster.h) and one that is given or needed is held to sr_geom_bytes(P).
UNRECORDED = [("sr_forward_render", "geom", "null", NO_DUPLICATES, ()), ("sr_forward_render", "geom", "null", NO_DUPLICATES_ONE_WAVE, ()),
              ("sr_forward_render", "geom", "short", NO_DUPLICATES, ()), ("sr_forward_render", "geom", "short", NO_GAUSSIANS, ()),
              ("sr_class_forward_render", "geom", "short", NO_DUPLICATES, ())]
# Two faults at once, recorded: sr_debug_pair_decisions is no backward call but looks at its buffers in the backward calls' order -- every
# NULL before every size, the geometry buffer first -- so a NULL geom beats a short binning.
DOUBLE_FAULTS = [("sr_debug_pair_decisions", "geom", "null", None, (("binning", "short"),))]


def faults(entry):
    """Every (argument, fault) of an entry point, in the order of its argument list."""
    every = [(b, f) for b in buffers_of(entry) for f in ("null", "short")] + [(q, "null") for q in pointers_of(entry)]
    return [(a, f) for a, f in every if (entry, a, f) not in AFTER_A_HIP_CALL]


class Scene:
    """The fixed scene and what keeps its memory alive; refusal(entry, argument, fault, case, also) makes one call -> (status, sr_last_error())."""

    def __init__(self, lib):
        self.lib = lib
        self.dummy = ctypes.create_string_buffer(64)
        p = self.p = ctypes.addressof(self.dummy)
        self.values = {
            "P": P, "D": D, "W": W, "H": H, "n_classes": N_CLASSES,
            "frame": _lib.SrFrame(H, W, 1.0, 1.0, 1.0, 0, 0, 0, p, p, p, p, 0, 0, 0, None),
            "g": _lib.SrGaussians(P, 0, 3, 0, p, p, p, p, None, p, None, None),   # scales + rotations, colors_precomp[P,3]
        }
        self.typed = {"num_rendered_host": ctypes.c_uint32(0), "grads": _lib.SrGradients(p, p, p, p, p, p, p, p)}
        self.need = {"geom": lib.sr_geom_bytes(P), "binning": lib.sr_binning_bytes(P, D, W, H), "image": lib.sr_image_bytes(W, H),
                     "class_image": lib.sr_class_image_bytes(W, H, N_CLASSES), "class_state": lib.sr_class_shared_bytes(P, W, H, N_CLASSES, D),
                     "workspace": lib.sr_backward_workspace_bytes(P, D, 3)}

    def refusal(self, entry, argument, fault, case=None, also=()):
        bad = {(argument, fault)} | {tuple(x) for x in also}
        values, args, case = dict(self.values), [], CASES[case]
        values["D"] = case.get("D", D)
        if "flags" in case:
            values["frame"] = _lib.SrFrame(H, W, 1.0, 1.0, 1.0, 0, 0, 0, self.p, self.p, self.p, self.p, 0, 0, case["flags"], None)
        if "P" in case:
            values["g"] = _lib.SrGaussians(case["P"], 0, 3, 0, self.p, self.p, self.p, self.p, None, self.p, None, None)
        need = dict(self.need, geom=self.lib.sr_geom_bytes(case.get("P", P)))
        for a in ARGUMENTS[entry]:
            if a in BUFFERS:
                args += [None if (a, "null") in bad else self.p, need[a] - 1 if (a, "short") in bad else BIG]
            elif a.startswith("@"):
                name = a[1:]
                typed = VIEWS[entry]() if name == "out" else self.typed.get(name)
                args.append(None if (name, "null") in bad else (ctypes.byref(typed) if typed is not None else self.p))
            else:
                v = values[a]
                args.append(ctypes.byref(v) if isinstance(v, ctypes.Structure) else v)
        if entry not in VIEWS:
            args.append(None)   # the stream
        return int(getattr(self.lib, entry)(*args)), self.lib.sr_last_error().decode()
