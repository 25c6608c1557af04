// oracle/shim/stb_image.h -- TEST INFRASTRUCTURE ONLY: the reference's colour header includes an image reader it does not use.
#pragma once
