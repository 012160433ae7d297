// rom_local_fused.hip -- bg_local_rom_limits / bg_local_rom_run (local POD, reference FEM/fem_burgers.py:979-1079): the
// LOCAL instantiations of rom_fused_kernel, whose body, launchers and entry points live in rom_fused.hip.
// They are compiled in a translation unit of their own: next to the POD instantiations they changed how the shared device
// helpers were inlined into those (rom_fused_kernel<8, 10, Galerkin> went from 12 to 300 bytes of scratch), and the POD
// kernels are meant to stay exactly what they were.
#define BG_ROM_FUSED_LOCAL_TU
#include "rom_fused.hip"
