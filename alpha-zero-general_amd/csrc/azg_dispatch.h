// azg_dispatch.h -- the device games and the run-time (game, variant) -> G dispatch, shared by the translation units that instantiate a
// kernel per game (azg.hip, azg_playout.hip).  Needs azg_host.h's fail() at the point of use.
#pragma once
#include "../../include/azg.h"
#include "game_splendor.hip.h"
#include "game_santorini.hip.h"
#include "game_azul.hip.h"
#include "game_minivilles.hip.h"
#include "game_abalone.hip.h"
#include "game_tlp.hip.h"
#include "game_botanik.hip.h"
#include "game_akropolis.hip.h"
#include "game_smallworld.hip.h"
#include "azg_host.h"

// ---- game dispatch --------------------------------------------------------------------------------------------------
#define AZG_DISPATCH(game, variant, ...)                                                         \
    do {                                                                                           \
        if ((game) == AZG_SPLENDOR && (variant) == 2) { using G = SplendorDev<2>; __VA_ARGS__; }          \
        else if ((game) == AZG_SPLENDOR && (variant) == 3) { using G = SplendorDev<3>; __VA_ARGS__; }     \
        else if ((game) == AZG_SPLENDOR && (variant) == 4) { using G = SplendorDev<4>; __VA_ARGS__; }     \
        else if ((game) == AZG_SANTORINI && (variant) == 1) { using G = SantoriniDev<1>; __VA_ARGS__; }   \
        else if ((game) == AZG_SANTORINI && (variant) == 11) { using G = SantoriniDev<11>; __VA_ARGS__; } \
        else if ((game) == AZG_AZUL) { using G = AzulDev; __VA_ARGS__; }                                   \
        else if ((game) == AZG_ABALONE && (variant) >= 1 && (variant) <= 3) { using G = AbaloneDevT<false>; __VA_ARGS__; } \
        else if ((game) == AZG_ABALONE && (variant) >= 5 && (variant) <= 7) { using G = AbaloneDevT<true>; __VA_ARGS__; }  \
        else if ((game) == AZG_MINIVILLES && (variant) == 2) { using G = MinivillesDev<2>; __VA_ARGS__; } \
        else if ((game) == AZG_MINIVILLES && (variant) == 3) { using G = MinivillesDev<3>; __VA_ARGS__; } \
        else if ((game) == AZG_MINIVILLES && (variant) == 4) { using G = MinivillesDev<4>; __VA_ARGS__; } \
        else if ((game) == AZG_TLP && (variant) == 3) { using G = TLPDev<3>; __VA_ARGS__; }               \
        else if ((game) == AZG_TLP && (variant) == 4) { using G = TLPDev<4>; __VA_ARGS__; }               \
        else if ((game) == AZG_TLP && (variant) == 5) { using G = TLPDev<5>; __VA_ARGS__; }               \
        else if ((game) == AZG_BOTANIK) { using G = BotanikDev; __VA_ARGS__; }                             \
        else if ((game) == AZG_AKROPOLIS && (variant) == 2) { using G = AkropolisDev<2>; __VA_ARGS__; }   \
        else if ((game) == AZG_AKROPOLIS && (variant) == 3) { using G = AkropolisDev<3>; __VA_ARGS__; }   \
        else if ((game) == AZG_AKROPOLIS && (variant) == 4) { using G = AkropolisDev<4>; __VA_ARGS__; }   \
        else if ((game) == AZG_SMALLWORLD && (variant) == 2) { using G = SmallworldDev<2>; __VA_ARGS__; } \
        else if ((game) == AZG_SMALLWORLD && (variant) == 3) { using G = SmallworldDev<3>; __VA_ARGS__; } \
        else if ((game) == AZG_SMALLWORLD && (variant) == 4) { using G = SmallworldDev<4>; __VA_ARGS__; } \
        else return fail("unsupported game/variant");                                              \
    } while (0)

static inline int norm_variant(int game, int variant) {
    if (game == AZG_SPLENDOR) return variant ? variant : 2;
    if (game == AZG_SANTORINI) return variant ? variant : 11;
    if (game == AZG_AZUL) return 2;
    if (game == AZG_MINIVILLES) return variant ? variant : 2;
    if (game == AZG_ABALONE)        // bits 0-1 the layout (0 = the default, Belgian Daisy), bit 2 dynamic komi; anything else is refused
        return (variant & ~7) ? -1 : ((variant & 3) ? variant : (variant | 1));
    if (game == AZG_TLP) return variant ? variant : 3;
    if (game == AZG_BOTANIK) return 2;
    if (game == AZG_AKROPOLIS) return variant ? variant : 2;
    if (game == AZG_SMALLWORLD) return variant ? variant : 2;
    return variant;
}
