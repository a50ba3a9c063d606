# tests/host_sim/crc.mk: the CRC32 roles (nlzm_amd/csrc/nlzm_crc.h) run on the CPU, every lane a fiber (xw_sim.cpp), under UBSan as
# decode_sim_san is (AddressSanitizer does not follow the fibers' hand-switched stacks: the harness puts PROT_NONE pages round every
# buffer instead).  TEST HARNESS ONLY.
SRC  = crc_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_crc.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: crc_sim_san
crc_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f crc_sim_san
