// oracle/shim/stb_image_write.h -- TEST INFRASTRUCTURE ONLY: the one writer the reference's colour header names; the harness
// writes no image, so it reports failure.
#pragma once

inline int stbi_write_png(const char *, int, int, int, const void *, int) { return 0; }
