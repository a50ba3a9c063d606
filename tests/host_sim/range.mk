# tests/host_sim/range.mk: the decoder role's prefix mode (nlzm_amd/csrc/nlzm_decode.h) and the gather role (nlzm_amd/csrc/nlzm_range.h) run
# on the CPU, every lane a fiber (xw_sim.cpp).  TEST HARNESS ONLY.  range_sim: the product's ring; range_sim_tiny: the smallest ring the
# decoder role allows, as decode.mk's (matches come from "memory" and are cut there).
SRC  = range_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_decode.h ../../nlzm_amd/csrc/nlzm_range.h ../../nlzm_amd/csrc/nlzm_host_decode.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: range_sim range_sim_tiny
range_sim: $(DEPS)
	g++ $(CXXFLAGS) -o $@ $(SRC)
range_sim_tiny: $(DEPS)
	g++ $(CXXFLAGS) -DNLZM_DEC_RING=512 -o $@ $(SRC)
clean:
	rm -f range_sim range_sim_tiny
