// wdl_repitch_driver.cpp -- the block loop of Audio::repitch (Audio/AudioTemporal.cpp:251-296) around the reference's own WDL_Resampler,
// for make_wdl_repitch.py.  Compiled there together with the reference's WDL/resample.cpp into a temporary directory; nothing built from
// it is kept.  Channel-major buffers in and out (float[ch][frames]), like the C ABI of include/flanhip.h.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "WDL/resample.h"

extern "C" {

// AudioTemporal.cpp:252 with FunctionSample<float>::accumulate() of a vector (std::accumulate from float()), the product and ceil in fp32
int64_t wdl_repitch_out_frames( const float * inv, int64_t count, int granularity )
	{
	const float sum = std::accumulate( inv, inv + count, float() );
	const int frames = std::ceil( sum * granularity );
	return frames;
	}

// quality: 0 Sinc, 1 Linear, 2 Uninterpolated (WDLResampleType's order).  Returns the number of blocks; wanted[b] is what
// ResamplePrepare asked for in block b and delivered[b] what ResampleOut returned (the first wanted_cap of each are stored).
int64_t wdl_repitch( const float * x, int num_channels, int in_frames, float sample_rate, const float * inv, int granularity, int quality,
	float * out, int num_out_frames, int32_t * wanted_out, int32_t * delivered_out, int64_t wanted_cap )
	{
	WDL_Resampler rs;
	if( quality == 0 ) rs.SetMode( true, 0, true, 64 );
	else if( quality == 1 ) rs.SetMode( true, 1, false );
	else rs.SetMode( false, 0, false );

	std::vector<float> rsoutbuf( size_t( num_channels ) * granularity );
	std::fill( out, out + size_t( num_channels ) * num_out_frames, 0.0f );

	int64_t blocks = 0;
	int in_frame = 0, out_frame = 0;
	while( in_frame < in_frames )
		{
		const double factor_to_use = inv[ int( std::floor( in_frame / float( granularity ) ) ) ];
		rs.SetRates( sample_rate, double( sample_rate ) * factor_to_use );
		WDL_ResampleSample * rsinbuf = nullptr;
		const int wanted = rs.ResamplePrepare( granularity, num_channels, &rsinbuf );

		for( int channel = 0; channel < num_channels; ++channel )
			for( int frame = 0; frame < wanted; ++frame )
				rsinbuf[ frame * num_channels + channel ] = in_frame + frame < in_frames ? x[ size_t( channel ) * in_frames + in_frame + frame ] : 0.0f;

		const int delivered = rs.ResampleOut( rsoutbuf.data(), wanted, granularity, num_channels );

		for( int channel = 0; channel < num_channels; ++channel )
			for( int frame = 0; frame < granularity; ++frame )
				if( out_frame + frame < num_out_frames )
					out[ size_t( channel ) * num_out_frames + out_frame + frame ] = rsoutbuf[ frame * num_channels + channel ];

		if( blocks < wanted_cap ) { wanted_out[blocks] = wanted; delivered_out[blocks] = delivered; }
		++blocks;
		out_frame += granularity;
		in_frame += wanted;
		}
	return blocks;
	}

}
