# tests/host_sim/planes.mk: the byte-plane role (nlzm_amd/csrc/nlzm_planes.h) run on the CPU, every lane a fiber (xw_sim.cpp), under UBSan as
# cut_sim_san is (AddressSanitizer does not follow the fibers' hand-switched stacks: the harness puts PROT_NONE pages round every source
# and guard bytes round every destination instead).  TEST HARNESS ONLY.
SRC  = planes_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_planes.h ../../nlzm_amd/csrc/nlzm_planes_plan.h ../../nlzm_amd/csrc/nlzm_range.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: planes_sim_san
planes_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f planes_sim_san
