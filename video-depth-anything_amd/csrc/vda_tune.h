// Route and schedule knobs.  The product library (`make` -> libvda.so) keeps no mutable global state:
// every knob below is a compile-time constant at its automatic value, and the vda_debug_* entry points
// do not exist.  The tuning build (`make tune` -> build/tune/libvda.so, -DVDA_TUNING) turns the knobs
// into process-global variables set through the entry points of include/vda_tune.h, for A/B runs and
// for the tests that compare the alternative kernel routes with the default one.
//
// VDA_KNOB: a knob of one file.  A knob read by several files is declared in a shared header with
// VDA_KNOB_DECL (product: the constant itself; tuning: extern) and defined once, in the file that owns
// its vda_debug_* setter, with VDA_KNOB_DEF (product: only checks that the two values agree).
#pragma once
#ifdef VDA_TUNING
#define VDA_KNOB(type, name, value) type name = value
#define VDA_KNOB_DECL(type, name, value) extern type name
#define VDA_KNOB_DEF(type, name, value) type name = value
#else
#define VDA_KNOB(type, name, value) constexpr type name = value
#define VDA_KNOB_DECL(type, name, value) constexpr type name = value
#define VDA_KNOB_DEF(type, name, value) static_assert(name == value, "knob declared with another value")
#endif
