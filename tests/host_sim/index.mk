# tests/host_sim/index.mk: the sidecar index's parser, validators and writer (nlzm_amd/csrc/nlzm_index.h) in a program of its own, under
# AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_index_sim.py).
DEPS = index_sim.cpp ../../nlzm_amd/csrc/nlzm_index.h
all: index_sim_san
index_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ index_sim.cpp
clean:
	rm -f index_sim_san
