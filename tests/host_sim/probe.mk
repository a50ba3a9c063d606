# tests/host_sim/probe.mk: the xw.h probe role (tests/xw_probe/xw_probe.h) run on the CPU, every lane a fiber (xw_sim.cpp), under UBSan as
# crc_sim_san is (AddressSanitizer does not follow the fibers' hand-switched stacks: the harness puts a PROT_NONE page behind every
# table instead).  TEST HARNESS ONLY.
SRC  = xw_probe_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../xw_probe/xw_probe.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: xw_probe_sim_san
xw_probe_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f xw_probe_sim_san
