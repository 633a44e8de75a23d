"""Slot numbering of the s8-48 layout (the 8-bit saved tensors of the 48-point training kernels, csrc/mlp_geo48.h TrainLayout48), for
the tests that unpack those buffers with dn_mlp_unpack: slots count 64-feature units per 16-point group.  The 32-point layouts' slots
come from nerf._train._slots."""


def s8_slots(depth, width, viewdirs):
    """(activation slots, gradient slots, units of one hidden vector) of a depth x width network in the s8-48 layout."""
    khu = width // 64
    s8 = {"xyz": 0, "dir": 1, "layer1": 1 + (1 if viewdirs else 0)}
    s8["trunk0"] = s8["layer1"] + khu
    s8["feat"] = s8["trunk0"] + (depth - 1) * khu
    s8["dirout"] = s8["feat"] + (khu if viewdirs else 0)
    g8 = {"dirout": 0, "feat": (width // 128) if viewdirs else 0}
    g8["trunk0"] = g8["feat"] + (khu if viewdirs else 0)
    g8["layer1"] = g8["trunk0"] + (depth - 1) * khu
    g8["out"] = g8["layer1"] + khu
    return s8, g8, khu
